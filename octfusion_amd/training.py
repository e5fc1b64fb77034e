"""Training step of the first (lr) diffusion stage -- SURVEY 8f-4.

Mirror of the reference's optimize_parameters for stage_flag == "lr" (octfusion_model_union.py:242-269, 271-292,
478-487): noise the split codes at a random log-SNR, predict x0, MSE, backward, AdamW, EMA.  Forward and backward
run on libofx (octfusion_amd/backward.py); the optimiser and EMA are one elementwise kernel launch per parameter, or,
with ``fused=True``, one multi-tensor call (csrc/ofx_train.hip) and a loss that stays on the device.
"""
import torch

from . import backward as BW
from . import ops, sampler
from ._lib import OfxAdamRow, call, lib, ptr, stream


class AdamW:
    """torch.optim.AdamW (the reference's optimiser, octfusion_model_union.py:142) on ofx_adamw_step."""

    def __init__(self, named_params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, sync=True):
        self.params = dict(named_params)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.step_count = 0
        self.state = {k: (torch.zeros_like(p.data), torch.zeros_like(p.data)) for k, p in self.params.items()}
        if sync:
            self.sync_()

    @torch.no_grad()
    def sync_(self, src=0):
        """Under torch.distributed: every rank takes rank `src`'s parameters and optimiser state (what wrapping the net
        in DistributedDataParallel does at construction for the reference, octfusion_model_union.py:185-196) -- ranks
        that were seeded differently would otherwise average gradients of different models, silently."""
        import torch.distributed as td
        from . import dist as D
        if not D._active():
            return 0
        keys = sorted(self.params)
        tensors = [self.params[k].data for k in keys] + [s for k in keys for s in self.state[k]]
        flat = torch.cat([t_.reshape(-1).float() for t_ in tensors])
        td.broadcast(flat, src=src)
        off = 0
        for t_ in tensors:
            n = t_.numel()
            t_.copy_(flat[off:off + n].view_as(t_))
            off += n
        for k in keys:
            _bump(self.params[k])
        step = torch.tensor([self.step_count], dtype=torch.int64, device=flat.device)
        td.broadcast(step, src=src)
        self.step_count = int(step.item())
        return flat.numel() * 4

    @torch.no_grad()
    def step(self, grads, ema=None, ema_rate=None, fused=False, source=None):
        """One AdamW update.  Under torch.distributed (one process per GPU) the gradients are first averaged over the
        ranks (dist.all_reduce_mean_: what DistributedDataParallel does for the reference).

        fused=True: one ofx_adamw_ema_multi call over the optimiser's parameters instead of a launch per tensor (the
        same arithmetic, the same bits).  With `ema` -- a module with the parameter names of the net the optimiser was
        built from -- and `ema_rate`, the EMA of the trained tensors is folded into that call, and one more EMA-only
        call covers the parameters of `ema` the optimiser does not own (the frozen earlier stages: the reference's EMA
        runs over the whole net); their live values are taken from `source`, the net itself."""
        from . import dist as D
        D.all_reduce_mean_(grads)
        self.step_count += 1
        if fused:
            return self._step_fused(grads, ema, ema_rate, source)
        if ema is not None:
            raise ValueError('AdamW.step: the EMA is folded in only with fused=True (use ema_update otherwise)')
        for k, p in self.params.items():
            g = grads.get(k)
            if g is None:         # no gradient this step: torch.optim skips the parameter entirely (no decay either)
                continue
            g = g.contiguous()
            assert g.shape == p.shape, (k, g.shape, p.shape)
            m, v = self.state[k]
            call('ofx_adamw_step', ptr(p.data), ptr(g), ptr(m), ptr(v), p.numel(), self.lr, self.betas[0], self.betas[1],
                 self.eps, self.weight_decay, self.step_count, stream())
            _bump(p)              # the kernel wrote behind torch's back: bump the version so packed-weight caches repack

    def _step_fused(self, grads, ema, ema_rate, source):
        if ema is not None and ema_rate is None:
            raise ValueError('AdamW.step: ema needs ema_rate')
        ema_params = dict(ema.named_parameters()) if ema is not None else {}
        rows, keep, written = [], [], []
        for k, p in self.params.items():
            g = grads.get(k)
            e = ema_params.pop(k, None)
            if g is None and e is None:
                continue
            assert p.is_contiguous(), k
            m = v = None
            if g is not None:
                g = g.contiguous()
                assert g.shape == p.shape and g.dtype == torch.float32, (k, g.shape, p.shape, g.dtype)
                m, v = self.state[k]
                keep.append(g)                  # the contiguous copy lives until the call is issued
                written.append(p)
            if e is not None:
                assert e.shape == p.shape and e.is_contiguous(), k
                written.append(e)
            rows.append((ptr(p.data), ptr(g), ptr(m), ptr(v), ptr(e), p.numel()))
        self._multi(rows, ema_rate)
        if ema_params:                          # what the optimiser does not own: EMA only, in one more call
            if source is None:
                raise ValueError('AdamW.step: `ema` has parameters outside the optimiser (%s, ...): pass the net as '
                                 '`source`' % next(iter(ema_params)))
            live = dict(source.named_parameters())
            rows = []
            for k, e in ema_params.items():
                p = live[k]
                assert e.shape == p.shape and e.is_contiguous() and p.is_contiguous(), k
                rows.append((ptr(p.data), None, None, None, ptr(e.data), p.numel()))
                written.append(e)
            self._multi(rows, ema_rate)
        _bump_all(written)

    def _multi(self, rows, ema_rate):
        table = (OfxAdamRow * max(len(rows), 1))(*rows)
        call('ofx_adamw_ema_multi', table, len(rows), self.lr, self.betas[0], self.betas[1], self.eps,
             self.weight_decay, self.step_count, 0.0 if ema_rate is None else ema_rate, stream())

    def state_dict(self):
        """{'step', 'state': {name: (exp_avg, exp_avg_sq)}} -- what checkpoint.save_ckpt stores under 'opt'."""
        return {'step': self.step_count, 'state': {k: (m.clone(), v.clone()) for k, (m, v) in self.state.items()}}

    def load_state_dict(self, sd):
        self.step_count = int(sd.get('step', 0))
        for k, (m, v) in sd.get('state', {}).items():
            if k in self.state:
                self.state[k][0].copy_(m)
                self.state[k][1].copy_(v)


def _bump(p):
    """Mark a tensor written by a libofx kernel as modified (what an in-place torch op would do) without
    launching one."""
    torch._C._increment_version(p)


def _bump_all(tensors):
    """_bump for a list in one call.  torch._C._increment_version takes an iterable of tensors; handed a single tensor
    it iterates over that tensor's rows (one unbind per call, ~0.2 ms on the device: 60 ms of host time a step over a
    union net's 327 tensors, tools/train_step_probe.py), which the per-tensor path still pays."""
    try:
        torch._C._increment_version(list(tensors))
    except TypeError:                     # a torch whose _increment_version takes one tensor
        for t in tensors:
            _bump(t)


def trainable_parameters(net, stage):
    """The parameters the reference optimises in `stage` ('lr' | 'hr' | 'feature'): only that stage's own net --
    the earlier stages are frozen (requires_grad False, octfusion_model_union.py:127-142,
    octfusion_model_union_3t.py:53-72) and AdamW is built from the trainable ones only."""
    prefix = {'lr': 'unet_lr.', 'hr': 'unet_hr.', 'feature': 'unet_feature.'}[stage]
    return {k: p for k, p in net.named_parameters() if k.startswith(prefix)}


@torch.no_grad()
def ema_update(ema_module, module, beta):
    """ldm_diffusion_util.py:50-53."""
    for pe, p in zip(ema_module.parameters(), module.parameters()):
        call('ofx_ema_update', ptr(pe.data), ptr(p.data), p.numel(), beta, stream())
        _bump(pe)


def mse_grad(y, target):
    """ofx_mse_grad: (loss, dy) of mean((y - target)^2) -- dy = (y - target) * (2 / n) as torch computes it in fp32, the
    loss a 0-d fp64 device tensor (fp64 sum in a fixed order; nothing is read back)."""
    y, target = y.contiguous(), target.contiguous()
    assert y.shape == target.shape and y.dtype == target.dtype == torch.float32, (y.shape, target.shape)
    n = y.numel()
    dy = torch.empty_like(y)
    partials = torch.empty(lib().ofx_mse_grad_partials(n), dtype=torch.float64, device=y.device)
    loss = torch.empty((), dtype=torch.float64, device=y.device)
    call('ofx_mse_grad', ptr(y), ptr(target), ptr(dy), ptr(partials), ptr(loss), n, stream())
    return loss, dy


def _loss_and_dy(box, target, fused):
    """dy_fn of a stage step: leaves the loss in box['loss'] -- a python float (one host read), or with `fused` the
    0-d device tensor of mse_grad."""
    def dy_fn(y):
        if fused:
            box['loss'], dy = mse_grad(y, target)
            return dy
        diff = y - target
        box['loss'] = float((diff * diff).mean())
        return diff * (2.0 / diff.numel())
    return dy_fn


def _optimise(opt, grads, net, ema, ema_rate, fused):
    if fused:
        opt.step(grads, ema=ema, ema_rate=ema_rate, fused=True, source=net)
        return
    opt.step(grads)
    if ema is not None:
        ema_update(ema, net, ema_rate)


@torch.no_grad()
def lr_stage_step(net, opt, split_small, times=None, noise=None, label=None, ema=None, ema_rate=0.999, fused=False):
    """One optimisation step of the lr stage on a batch of split codes [B, 8, S, S, S] (values in {-1, +1}).
    net: graph_unet_lr.UNet3DModel.  Returns the loss (python float).  fused=True: loss and gradient come from
    ofx_mse_grad, optimiser and EMA are the multi-tensor call, and the loss is returned as a 0-d device tensor -- the
    step then waits for the device nowhere, provided `times` is given on the CPU."""
    B = split_small.shape[0]
    dev = split_small.device
    if times is None:
        times = torch.rand(B, device=dev)
    if noise is None:
        noise = torch.randn_like(split_small)
    log_snr = sampler.beta_linear_log_snr(times.cpu()).float().to(dev)
    alpha, sigma = sampler.log_snr_to_alpha_sigma(log_snr)
    noised = alpha.view(B, 1, 1, 1, 1) * split_small + sigma.view(B, 1, 1, 1, 1) * noise
    # the lr net takes cat(x, x_self_cond); training passes no self-conditioning (zeros), graph_unet_lr.py:198-204
    x = torch.cat((noised, torch.zeros_like(noised)), dim=1)
    rows = ops.voxel2octree_cf(x.float(), net.full_depth)
    target = ops.voxel2octree_cf(split_small.float(), net.full_depth)
    box = {}
    _, _, grads = BW.lr_unet_forward_backward(net, rows, B, log_snr, _loss_and_dy(box, target, fused), label=label)
    _optimise(opt, grads, net, ema, ema_rate, fused)
    return box['loss']


@torch.no_grad()
def hr_stage_step(net, opt, codes, doctree, depth, times=None, noise=None, label=None, ema=None, ema_rate=0.999,
                  stage='hr', df_type='eps', fused=False):
    """One optimisation step of a sparse stage (octfusion_model_union.py:242-269 / octfusion_model_union_3t.py):
    stage 'hr' = the hr net with the lr net nested, stage 'feature' = the feature net with the hr net nested;
    df_type 'eps' regresses the noise, 'x0' the clean data.  data [N, C] lives on the depth-`depth` dual graph
    (latent codes from GraphVAE.encode, or split codes); net = the union UNet3DModel; `opt` holds the parameters
    under their union state_dict names.  Returns the loss; fused=True as in lr_stage_step."""
    B = doctree.batch_size
    dev = codes.device
    if times is None:
        times = torch.rand(B, device=dev)
    if noise is None:
        noise = torch.randn_like(codes)
    log_snr = sampler.beta_linear_log_snr(times.cpu()).float().to(dev)
    alpha, sigma = sampler.log_snr_to_alpha_sigma(log_snr)
    bid = doctree.batch_id(depth)
    noised = (alpha[bid].unsqueeze(1) * codes + sigma[bid].unsqueeze(1) * noise).contiguous()
    box = {}

    target = noise if df_type == 'eps' else codes
    dy_fn = _loss_and_dy(box, target, fused)
    outer, nested = ('unet_hr', 'unet_lr') if stage == 'hr' else ('unet_feature', 'unet_hr')
    _, _, g_o, _g_nested = BW.hr_unet_forward_backward(getattr(net, outer), noised, doctree, getattr(net, nested),
                                                      log_snr, dy_fn, label=label)
    # only the stage's own net is trained: the nested earlier-stage net is frozen in the reference
    # (octfusion_model_union.py:127-142, octfusion_model_union_3t.py:53-72), so its gradients are dropped and
    # parameters without a gradient are skipped by the optimiser (torch's grad=None behaviour: no update, no decay)
    grads = {outer + '.' + k: v for k, v in g_o.items()}
    _optimise(opt, grads, net, ema, ema_rate, fused)
    return box['loss']
