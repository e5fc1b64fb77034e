"""Evaluation-metric kernels on the device (csrc/ofx_metrics.hip), timed with HIP events, against their VALU issue
roofs (MI355X_MICROARCH constants: 256 CUs x 4 SIMDs, a wave64 VALU issue every 4 cycles per SIMD = 16 lanes / clock,
v_exp_f32 and v_sqrt_f32 8 cycles; peak clock 2.4 GHz).

  * Chamfer: the union NN matrix at N = 2600 clouds (1.3 k references + 1.3 k samples), n = 2048: one launch, N^2 n^2
    point pairs at 3 issues per pair (direct differences, packed f32: 3 v_pk_add + v_pk_mul + 2 v_pk_fma per two
    pairs; the min costs another 0.5 in the shipped kernel).
  * EMD: a 256 x 256 matrix at n = 2048, extrapolated to the category run (M_rr + M_rs + M_ss = 3 x 1300^2 ordered
    pairs); per point pair and level: passes 1 and 2 cost 3 + 0.5 (level) + 2 (exp) + 0.5 (fma) issue slots, pass 3
    3 + 0.5 + 2 (exp) + 2 (sqrt) + 1.5.
  * The reference's loop (_pairwise_EMD_CD_: one sample against 256-reference batches, three calls for 1-NNA) on the
    same kernels: a few sample rows timed, extrapolated to the same matrices.

    python tools/metrics_probe.py --out profiles/metrics/metrics_probe.json [--quick]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from octfusion_amd import _lib, metrics

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--quick', action='store_true', help='small sizes (for a kernel-trace run)')
args = ap.parse_args()
torch.set_grad_enabled(False)
_lib.require_device()
dev = torch.device('cuda:0')
CLOCK, ROOF_LANES = 2.4e9, 256 * 4 * 16
N_CAT = 1300
N_U, N_E, N_PTS = (260, 32, 2048) if args.quick else (2600, 256, 2048)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / reps


g = torch.Generator(device=dev).manual_seed(0)
U = (torch.rand(N_U, N_PTS, 3, device=dev, generator=g) * 2 - 1).contiguous()
rows = {}

# ---- Chamfer: the union matrix in one launch
t_nn = timed(lambda: metrics.nn_matrix(U, U), 1 if not args.quick else 3)
pairs = float(N_U) ** 2 * N_PTS ** 2
rows['chamfer_union'] = dict(N=N_U, n=N_PTS, seconds=t_nn, point_pairs=pairs,
                             roof_seconds_3_issues=pairs * 3 / (ROOF_LANES * CLOCK),
                             frac_of_roof_3_issues=pairs * 3 / (ROOF_LANES * CLOCK) / t_nn,
                             frac_of_roof_3p5_issues=pairs * 3.5 / (ROOF_LANES * CLOCK) / t_nn)
print(json.dumps(rows['chamfer_union']), flush=True)

# ---- EMD: an N_E x N_E block
X = U[:N_E].contiguous()
t_emd = timed(lambda: metrics.emd_matrix(X, X), 1)
issues = float(N_E) ** 2 * N_PTS ** 2 * 9 * ((3 + 0.5 + 2 + 0.5) * 2 + (3 + 0.5 + 2 + 2 + 1.5))
cat_pairs = 3 * N_CAT ** 2
rows['emd_block'] = dict(N=N_E, n=N_PTS, seconds=t_emd, seconds_per_pair=t_emd / N_E ** 2,
                         roof_seconds=issues / (ROOF_LANES * CLOCK), frac_of_issue_roof=issues / (ROOF_LANES * CLOCK) / t_emd,
                         category_pairs=cat_pairs, category_seconds_extrapolated=t_emd / N_E ** 2 * cat_pairs)
print(json.dumps(rows['emd_block']), flush=True)

# ---- the reference's loop on the same kernels: one sample row against 256-reference batches
R = U[:N_U // 2].contiguous()
n_rows = 4


def ref_loop_row(s, emd):
    x = R[s:s + 1]
    for b0 in range(0, R.shape[0], 256):
        rb = R[b0:b0 + 256]
        metrics.nn_matrix(x, rb)
        metrics.nn_matrix(rb, x)
        if emd:
            metrics.emd_matrix(x, rb)


t_row_cd = timed(lambda: [ref_loop_row(s, False) for s in range(n_rows)], 1) / n_rows
t_row_emd = timed(lambda: [ref_loop_row(s, True) for s in range(min(n_rows, 2))], 1) / min(n_rows, 2) - t_row_cd
nr = R.shape[0]
rows['reference_loop'] = dict(refs=nr, n=N_PTS, seconds_per_sample_row_cd=t_row_cd,
                              seconds_per_sample_row_emd=t_row_emd,
                              union_matrix_equivalent_seconds_cd=t_row_cd * (2 * nr) * (2 * nr) / nr,
                              union_launch_seconds_cd=t_nn * (2 * nr / N_U) ** 2,
                              note='the reference computes rs, rr and ss (and rs again for COV/MMD): '
                                   '4 calls of N rows against N references')
print(json.dumps(rows['reference_loop']), flush=True)
res = dict(device=torch.cuda.get_device_name(0), clock_assumed_hz=CLOCK, rows=rows)
if args.out:
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
