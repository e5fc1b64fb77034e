"""The float64 metrics oracle (tests/metrics_oracle.py) on the CPU: pinned to the reference's own CPU path
(tests/golden/g_metrics.pt, made by tests/golden/make_metrics_golden.py) for Chamfer, lgan_mmd_cov, knn and the
CD results of compute_cov_mmd / compute_1_nna; the approximate EMD by cases whose answer is known and by its ratio to
the exact Hungarian EMD; the sampler by geometry and a chi-square test; the counter hash against the library's."""
import numpy as np
import pytest
import torch

import metrics_oracle as O

# ratio approxmatch / exact Hungarian EMD on the golden clouds (all 63 + 49 + 81 ordered pairs), measured on the CPU
# with this oracle: 1.094 .. 1.235 -- recorded with a margin
EMD_RATIO_BAND = (1.0, 1.3)


@pytest.fixture(scope='module')
def g(golden):
    return golden('g_metrics')


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_chamfer_matches_the_reference(g):
    R, S = g['R'].numpy(), g['S'].numpy()
    for i in range(3):
        d2 = O._pair_d2(S[i], R[i])          # distChamfer(a, b): P.min(1) is per point of b, P.min(2) per point of a
        assert rel(d2.min(0), g['dl'][i]) < 1e-6 and rel(d2.min(1), g['dr'][i]) < 1e-6
    assert rel(O.chamfer_matrix(R, S), g['M_rs_cd']) < 1e-6
    assert rel(O.chamfer_matrix(R), g['M_rr_cd']) < 1e-6
    assert rel(O.chamfer_matrix(S), g['M_ss_cd']) < 1e-6
    D = O.nn_matrix(R, S)
    assert rel(D + O.nn_matrix(S, R).T, g['M_rs_cd']) < 1e-6


def check_results(have, want, keys):
    for k in keys:
        if 'cov' in k:          # the reference stores COV through a float32 tensor
            assert abs(have[k] - want[k]) < 1e-7, k
        elif 'acc' in k:
            assert have[k] == pytest.approx(want[k], rel=1e-12, abs=0), k
        else:
            assert have[k] == pytest.approx(want[k], rel=1e-6), k


def test_reductions_match_the_reference(g):
    check_results(O.lgan_mmd_cov(g['M_rs_cd'].t().numpy()), g['lgan_cd'], ['lgan_mmd', 'lgan_cov', 'lgan_mmd_smp'])
    k = O.knn(g['M_rr_cd'].numpy(), g['M_rs_cd'].numpy(), g['M_ss_cd'].numpy())
    check_results(k, g['knn_cd'], ['acc', 'acc_t', 'acc_f'])
    # the EMD keys of the drivers: the oracle's reductions fed the reference's (Hungarian) matrices
    res = O.cov_mmd_from(g['M_rs_cd'].numpy(), g['M_rs_emd'].numpy())
    res.update(O.one_nna_from(*(g[k].numpy() for k in ('M_rr_cd', 'M_rs_cd', 'M_ss_cd', 'M_rr_emd', 'M_rs_emd',
                                                         'M_ss_emd'))))
    check_results(res, {**g['cov_mmd'], **g['one_nna']}, list(g['cov_mmd']) + list(g['one_nna']))


def test_cd_results_of_the_drivers_from_the_oracle_matrices(g):
    R, S = g['R'].numpy(), g['S'].numpy()
    rs = O.chamfer_matrix(R, S)
    res = O.cov_mmd_from(rs)
    res.update(O.one_nna_from(O.chamfer_matrix(R), rs, O.chamfer_matrix(S)))
    assert sorted(res) == sorted(k for k in list(g['cov_mmd']) + list(g['one_nna']) if 'CD' in k)
    check_results(res, {**g['cov_mmd'], **g['one_nna']}, list(res))


def test_emd_of_a_cloud_with_itself_is_zero():
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (64, 3))
    assert O.approxmatch_cost(x, x) < 1e-6


def test_emd_of_a_permuted_shifted_copy_is_the_shift():
    rng = np.random.default_rng(2)
    x = np.stack(np.meshgrid(*[np.arange(4) * 0.3] * 3, indexing='ij'), -1).reshape(-1, 3)    # 64 points, 0.3 apart
    delta = np.array([0.004, -0.003, 0.002])
    y = x[rng.permutation(len(x))] + delta
    assert O.approxmatch_cost(x, y) == pytest.approx(np.linalg.norm(delta), rel=1e-3)
    assert O.approxmatch_cost(y, x) == pytest.approx(np.linalg.norm(delta), rel=1e-3)


def test_emd_against_the_exact_hungarian_emd(g):
    R, S = g['R'].numpy(), g['S'].numpy()
    ratios = []
    for A, B, key in ((R, S, 'M_rs_emd'), (R, R, 'M_rr_emd'), (S, S, 'M_ss_emd')):
        E = O.emd_matrix(A, B)
        H = g[key].numpy()
        off = ~np.eye(len(A), len(B), dtype=bool) if A is B else np.ones_like(H, bool)
        ratios += list((E[off] / H[off]).ravel())
        if A is B:
            assert np.abs(np.diag(E)).max() < 1e-6
    lo, hi = min(ratios), max(ratios)
    assert EMD_RATIO_BAND[0] <= lo and hi <= EMD_RATIO_BAND[1], (lo, hi)


def fixture_mesh():
    """Eight triangles of very different areas (two of them in one plane) around a tetrahedron."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 0.5], [3, 1, 1], [-1, 0.2, 0.1], [0.3, -0.4, 2.0]],
                 np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3], [1, 4, 2], [0, 5, 2], [3, 6, 1], [5, 6, 0]], np.int32)
    return v, f


def test_sampler_points_lie_on_their_triangles():
    v, f = fixture_mesh()
    for normalize in (False, True):
        p, t = O.sample_surface(v, f, 5000, seed=3, shape=1, normalize=normalize)
        vv = v.astype(np.float64)
        if normalize:
            c, s = O.normalize_frame(v)
            vv = (vv - c) * s
        d = O.point_triangle_distance(p, vv[f[t, 0]], vv[f[t, 1]], vv[f[t, 2]])
        assert d.max() < 1e-12
    c, s = O.normalize_frame(v)
    vn = (v - c) * s
    assert np.allclose((vn.max(0) + vn.min(0)) / 2, 0, atol=1e-7) and abs((vn.max(0) - vn.min(0)).max() - 2) < 1e-6


def test_sampler_triangle_counts_follow_area():
    v, f = fixture_mesh()
    n = 40000
    _, t = O.sample_surface(v, f, n, seed=11, shape=0)
    v = v.astype(np.float64)
    area = np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    expect = n * area / area.sum()
    chi2 = float((((np.bincount(t, minlength=len(f)) - expect) ** 2) / expect).sum())
    assert chi2 < 24.32                       # chi-square, 7 degrees of freedom, p = 0.001
    # another seed and another shape id draw other points
    p0, _ = O.sample_surface(v, f, 64, seed=11, shape=0)
    assert not np.array_equal(p0, O.sample_surface(v, f, 64, seed=12, shape=0)[0])
    assert not np.array_equal(p0, O.sample_surface(v, f, 64, seed=11, shape=1)[0])


def test_barycentrics_are_uniform_and_reflected():
    i = np.arange(200000, dtype=np.uint64)
    iu = (O.hash_draw(5, 0, i, 1) >> np.uint64(40)).astype(np.int64)
    iw = (O.hash_draw(5, 0, i, 2) >> np.uint64(40)).astype(np.int64)
    u, w = iu / 2 ** 24, iw / 2 ** 24
    assert abs(u.mean() - 0.5) < 0.005 and abs(w.mean() - 0.5) < 0.005 and abs(np.corrcoef(u, w)[0, 1]) < 0.01
    p, _ = O.sample_surface(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]]), 20000,
                            seed=5, normalize=False)
    assert (p[:, 0] + p[:, 1] <= 1 + 1e-12).all() and abs(p[:, 0].mean() - 1 / 3) < 0.01


def test_library_hash_equals_the_oracle():
    from octfusion_amd import build, _lib
    build.build()
    L = _lib.lib()
    for seed, shape, point, draw in ((0, 0, 0, 0), (7, 3, 12345, 2), (2 ** 64 - 1, 2 ** 40, 2 ** 31, 1)):
        assert L.ofx_metrics_hash(seed, shape, point, draw) == int(O.hash_draw(seed, shape, point, draw))
    assert L.ofx_surface_sample_ws_bytes(0, 10) == 0 and L.ofx_surface_sample_ws_bytes(2, 100) >= 100 * 8


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_metrics_fail_loudly_without_gpu():
    from octfusion_amd import _lib, metrics
    with pytest.raises(_lib.OfxError):
        metrics.chamfer_matrix(torch.zeros(2, 8, 3))
    with pytest.raises(_lib.OfxError):
        metrics.sample_surface([fixture_mesh()])
