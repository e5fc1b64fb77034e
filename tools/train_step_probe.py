"""What the optimiser side of a training step costs, per-tensor launches against the multi-tensor call.

snet_uncond widths, shell-6 octrees, batch 8; stage hr (eps objective, EMA over the whole union net) and stage lr.
For each stage three arms run in one process, alternating: fused=False, fused=True, fused=False again -- the first and
the last are the same code (the per-tensor path, unchanged), so their difference is the run-to-run spread a
fused-against-plain difference has to beat.  Per arm, over --steps steps after --warmup:

  step_ms        wall clock per step around a window that ends in a device synchronise
  step_event_ms  the same window by HIP events
  issue_ms       host time per step until the step function returns (its last launch is issued); the plain step reads
                 the loss back, so for it this includes waiting for the device
  optim_ms       HIP events around the optimiser + EMA portion (training._optimise), mean per step
  optim_host_ms  host time of that portion
  launches       kernel launches of that portion per step: counted entry-point calls for the per-tensor path (one
                 launch each); for the multi-tensor call COMPUTED as ceil(rows with work / ofx_adamw_ema_multi_rows())

    python tools/train_step_probe.py [--steps 20] [--warmup 3] [--out profiles/train/train_step_probe.json]
"""
import argparse
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from octfusion_amd import _lib, configs, graph_unet_union as U, synthetic, training as TR
from octfusion_amd.dual_octree import DualOctree
from octfusion_amd.octree import split2octree_small


class OptimMeter:
    """Brackets training._optimise with HIP events and counts its launches."""

    def __init__(self):
        self.events, self.host, self.launches, self.on = [], 0.0, 0, False
        self._optimise, self._call, self._multi = TR._optimise, TR.call, TR.AdamW._multi
        meter = self

        def optimise(*a, **k):
            if not meter.on:
                return meter._optimise(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            meter._optimise(*a, **k)
            e1.record()
            meter.host += time.perf_counter() - t0
            meter.events.append((e0, e1))

        def call(name, *a):
            if meter.on and name in ('ofx_adamw_step', 'ofx_ema_update'):
                meter.launches += 1
            return meter._call(name, *a)

        def multi(opt, rows, ema_rate):
            if meter.on:
                per_launch = _lib.lib().ofx_adamw_ema_multi_rows()
                meter.launches += -(-sum(1 for r in rows if r[5] > 0) // per_launch)
            return meter._multi(opt, rows, ema_rate)
        TR._optimise, TR.call, TR.AdamW._multi = optimise, call, multi

    def reset(self, on):
        self.events, self.host, self.launches, self.on = [], 0.0, 0, on


def run_arm(meter, step, steps, warmup):
    meter.reset(False)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    meter.reset(True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    issue = 0.0
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        t = time.perf_counter()
        step()
        issue += time.perf_counter() - t
    e1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    optim = sum(a.elapsed_time(b) for a, b in meter.events) / steps
    out = dict(step_ms=wall / steps * 1e3, step_event_ms=e0.elapsed_time(e1) / steps, issue_ms=issue / steps * 1e3,
               optim_ms=optim, optim_host_ms=meter.host / steps * 1e3, launches=meter.launches / steps)
    meter.reset(False)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--out', default='profiles/train/train_step_probe.json')
    args = ap.parse_args(argv)
    _lib.require_device()
    dev = torch.device('cuda:0')
    torch.set_grad_enabled(False)
    cfg = configs.SNET_UNCOND
    B = args.batch
    split = synthetic.shell6_split(B).to(dev)
    doc = DualOctree(split2octree_small(split, 6, 4))
    codes = torch.randn(doc.total_num, 3, device=dev)
    gen = torch.Generator().manual_seed(0)
    meter = OptimMeter()
    result = dict(config='snet_uncond', batch=B, rows_depth6=int(doc.total_num), steps=args.steps, warmup=args.warmup,
                  stages={})

    def fresh():
        net = U.UNet3DModel(**configs.unet_params('snet_uncond', 'hr'))
        net.load_state_dict(synthetic.random_state_dict(net))
        net = net.to(dev).eval()
        return net, copy.deepcopy(net)

    for stage in ('hr', 'lr'):
        arms = []
        for fused in (False, True, False):
            net, ema = fresh()
            if stage == 'hr':
                opt = TR.AdamW(TR.trainable_parameters(net, 'hr'), lr=1e-4)

                def step():
                    return TR.hr_stage_step(net, opt, codes, doc, 6, times=torch.rand(B, generator=gen), ema=ema,
                                            df_type=cfg['df_type'][1], fused=fused)
            else:
                opt = TR.AdamW(dict(net.unet_lr.named_parameters()), lr=1e-4)

                def step():
                    return TR.lr_stage_step(net.unet_lr, opt, split, times=torch.rand(B, generator=gen),
                                            ema=ema.unet_lr, fused=fused)
            arm = run_arm(meter, step, args.steps, args.warmup)
            arm['fused'] = fused
            arm['trained_tensors'] = len(opt.params)
            arm['ema_tensors'] = sum(1 for _ in (ema if stage == 'hr' else ema.unet_lr).parameters())
            arms.append(arm)
            print('%s fused=%-5s step %.2f ms (events %.2f)  issue %.2f ms  optimiser+EMA %.3f ms (host %.3f)  %d launches'
                  % (stage, fused, arm['step_ms'], arm['step_event_ms'], arm['issue_ms'], arm['optim_ms'],
                     arm['optim_host_ms'], arm['launches']), flush=True)
            del net, ema, opt
        base = [a for a in arms if not a['fused']]
        result['stages'][stage] = dict(
            arms=arms, baseline_spread_ms={k: abs(base[0][k] - base[1][k]) for k in ('step_ms', 'issue_ms', 'optim_ms')})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(result, fh, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
