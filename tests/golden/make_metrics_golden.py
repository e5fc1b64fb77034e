"""Golden vectors of the reference's evaluation metrics (metrics/evaluation_metrics.py) -> tests/golden/g_metrics.pt.

CPU only, through refenv.py: the CUDA extension cannot load here, so the reference falls back to its own CPU paths --
distChamfer (:11-21) for Chamfer and the exact Hungarian emd_approx (:35-52) for EMD.  The clouds are float64, so the
reference's |x|^2 + |y|^2 - 2 x.y form keeps ~1e-13 relative accuracy.  Recorded: the clouds, distChamfer of three
pairs, the three _pairwise_EMD_CD_ matrices (:111-153), lgan_mmd_cov (:189-201) and knn (:157-186) of them, and
compute_cov_mmd / compute_1_nna (:204-238).

    python tests/golden/make_metrics_golden.py
"""
import contextlib
import io
import os

import numpy as np
import torch

import refenv

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'g_metrics.pt')
N_REF, N_SMP, N_PTS, BATCH = 7, 9, 48, 4


def clouds(rng, count):
    """Noisy shells of random boxes: distinct enough that nearest neighbours are unambiguous."""
    out = []
    for _ in range(count):
        half = rng.uniform(0.3, 1.0, 3)
        p = rng.uniform(-1, 1, (N_PTS, 3))
        ax = rng.integers(0, 3, N_PTS)
        p[np.arange(N_PTS), ax] = np.sign(p[np.arange(N_PTS), ax] + 1e-12)
        out.append(p * half + rng.normal(0, 0.02, (N_PTS, 3)) + rng.normal(0, 0.05, 3))
    return torch.from_numpy(np.stack(out))


def main():
    refenv.setup()
    with contextlib.redirect_stdout(io.StringIO()):
        import metrics.evaluation_metrics as EM          # prints the two fall-back notices
    rng = np.random.default_rng(2024)
    R, S = clouds(rng, N_REF), clouds(rng, N_SMP)
    dl, dr = EM.distChamfer(S[:3], R[:3])
    with contextlib.redirect_stderr(io.StringIO()):
        M_rs_cd, M_rs_emd = EM._pairwise_EMD_CD_(R, S, BATCH)
        M_rr_cd, M_rr_emd = EM._pairwise_EMD_CD_(R, R, BATCH)
        M_ss_cd, M_ss_emd = EM._pairwise_EMD_CD_(S, S, BATCH)
        cov = EM.compute_cov_mmd(S, R, BATCH)
        nna = EM.compute_1_nna(S, R, BATCH)

    def plain(d):
        return {k: float(v) for k, v in d.items()}
    g = dict(R=R, S=S, dl=dl, dr=dr,
             M_rs_cd=M_rs_cd, M_rs_emd=M_rs_emd, M_rr_cd=M_rr_cd, M_rr_emd=M_rr_emd, M_ss_cd=M_ss_cd,
             M_ss_emd=M_ss_emd,
             lgan_cd=plain(EM.lgan_mmd_cov(M_rs_cd.t())),
             knn_cd={k: float(v) for k, v in EM.knn(M_rr_cd, M_rs_cd, M_ss_cd, 1, sqrt=False).items()},
             cov_mmd=plain(cov), one_nna=plain(nna))
    torch.save(g, OUT)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
