"""tests/train_oracle.py on the host: equal to the project's oracles where they overlap (oracle/loss.py with autograd,
oracle/points.py on two small clouds, oracle/modules.dual_octree_group_norm with autograd at count_eps = eps); its float32
evaluation inside the bounds the device tests use; the confident-logit table that made ofx_octree_ce a softplus; and the
count_eps terms of the GroupNorm backward shown to matter where the device test says they do."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gn_oracle as GN
import train_oracle as T
from glue_oracle import U, assert_close


def test_imports_nothing_from_the_package():
    import ast
    import inspect
    names = set()
    for node in ast.walk(ast.parse(inspect.getsource(T))):
        if isinstance(node, ast.Import):
            names |= {a.name.split('.')[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or '').split('.')[0])
    assert names == {'numpy', 'torch', 'glue_oracle', 'gn_oracle'}


# ------------------------------------------------------------------------------------------------ against oracle/loss.py
class _Tree:
    def __init__(self, child):
        self.child = torch.as_tensor(child)

    def nempty_mask(self, d):
        return self.child >= 0


def test_cross_entropy_equals_the_oracle():
    from oracle import loss as OL
    logits, child = T.ce_case_rows('mix', 5000, 3)
    with torch.enable_grad():
        lg = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
        out = OL.octree_loss({4: lg}, _Tree(child))
        (out['loss_4'] * 0.37 * len(child)).backward()
    ce, S = T.ce_rows(logits, child)
    loss = float(out['loss_4'].detach())
    assert abs(ce.mean() - loss) <= 1e-13 * loss
    assert T.ce_hits(logits, child) / len(child) == pytest.approx(float(out['accu_4']), abs=1e-7)
    assert T.ce_hits(logits, child) == int(torch.tensor(logits).argmax(1).eq(torch.tensor(T.ce_labels(child))).sum())
    want, Sg, c = T.ce_grad(logits, child, 0.37)
    # autograd forms softmax - onehot: exact to 2^-53 of 1; dscale is the fp32 0.37 here (what the C ABI carries) and
    # the double 0.37 there: U relative
    assert np.all(np.abs(want - lg.grad.numpy()) <= U * np.abs(want) + 4 * 2.0 ** -53)
    ties = logits[:, 0] == logits[:, 1]
    assert ties.sum() >= 5 and np.all(np.abs(np.abs(want[ties]) - 0.5 * np.float32(0.37)) < 1e-12)


def test_sdf_reg_equals_the_oracle():
    from oracle import loss as OL
    g = np.random.default_rng(4)
    n = 1001
    sdf, sg = g.standard_normal(n).astype(np.float32), g.standard_normal(n).astype(np.float32)
    grad, gg = g.standard_normal((n, 3)).astype(np.float32), g.standard_normal((n, 3)).astype(np.float32)
    with torch.enable_grad():
        s, gr = torch.tensor(sdf, requires_grad=True), torch.tensor(grad, requires_grad=True)
        o = OL.sdf_reg_loss(s.double(), gr.double(), torch.tensor(sg).double(), torch.tensor(gg).double())
        (o['grad_loss'] + o['sdf_loss']).backward()
    (sum_g, sum_s), dsdf, dgrad = T.sdf_reg(sdf, grad, sg, gg, 200.0, 1.0)
    # the oracle squares the float64 difference, the kernel the fp32 one: 2 U relative per term
    assert abs(sum_g / (3 * n) - float(o['grad_loss'])) <= 4 * U * float(o['grad_loss'])
    assert abs(200.0 * sum_s / n - float(o['sdf_loss'])) <= 4 * U * float(o['sdf_loss'])
    assert np.abs(dsdf - s.grad.numpy()).max() <= 4 * U * np.abs(dsdf).max()
    assert np.abs(dgrad - gr.grad.numpy()).max() <= 4 * U * np.abs(dgrad).max()


@pytest.mark.parametrize('with_noise', [True, False])
def test_posterior_equals_the_oracle(with_noise):
    from oracle import loss as OL
    E = 3
    params, noise, dz = T.posterior_case(500, E, 8)
    with torch.enable_grad():
        pr = torch.tensor(params, dtype=torch.float64, requires_grad=True)
        nz = torch.tensor(noise, dtype=torch.float64) if with_noise else torch.zeros(500, E, dtype=torch.float64)
        z_o, kl_o = OL.posterior(pr, nz)
        ((z_o * torch.tensor(dz, dtype=torch.float64)).sum() + 0.1 * kl_o.sum()).backward()
    (z, S_z), (kl, S_kl) = T.posterior(params, noise if with_noise else None, E)
    assert_close(torch.tensor(z), z_o, S_z, 1e-6, 'z')
    assert_close(torch.tensor(kl), kl_o, S_kl, 1e-6, 'kl')
    (dm, S_m), (dl, S_l) = T.posterior_bwd(params, noise if with_noise else None, dz, E, 0.1)
    # kl_scale is the fp32 0.1 in the closed form (what the C ABI carries) and the double 0.1 in autograd: 1 U
    assert_close(torch.tensor(dm), pr.grad[:, :E], S_m, 1.0, 'dmean')
    assert_close(torch.tensor(dl), pr.grad[:, E:], S_l + T.TINY, 1.0, 'dlogvar')
    sp = T.logvar_specials()
    blocked = np.array([0, 0, 1, 0, 0, 1, 1, 1, 0], dtype=bool)          # one ulp outside and +-40: no gradient
    assert np.array_equal(params.reshape(-1, 2 * E)[:, E:].reshape(-1)[:len(sp)], sp)
    got = dl.reshape(-1)[:len(sp)]
    assert np.all(got[blocked] == 0) and (not with_noise or np.all(got[~blocked] != 0))
    assert np.all(pr.grad[:, E:].reshape(-1)[:len(sp)].numpy()[blocked] == 0)


# ------------------------------------------------------------------------------------------------ against oracle/points.py
@pytest.mark.parametrize('depth,full_depth', [(5, 2), (6, 3)])
def test_points_equal_the_oracle(depth, full_depth):
    """two clouds of 700 and 300 points: keys, children of every depth and the 'ND' feature"""
    from oracle import points as OP
    g = torch.Generator().manual_seed(depth)
    clouds = [torch.rand(700, 3, generator=g) * 1.6 - 0.8, torch.rand(300, 3, generator=g) * 0.9 - 0.2]
    normals = [F.normalize(torch.randn(len(c), 3, generator=g)) for c in clouds]
    merged, feat = OP.points2octree_batch(clouds, normals, depth, full_depth)
    pts, nrm = torch.cat(clouds).numpy(), torch.cat(normals).numpy()
    batch = np.repeat([0, 1], [700, 300])
    sk, si = T.points_sort(T.points_keys(pts, batch, depth), np.arange(1000))
    fine = merged.keys[depth][merged.children[depth] >= 0].numpy()
    assert np.array_equal(np.unique(sk), fine)
    for d in range(full_depth, depth + 1):
        label = T.label_from_points(sk, merged.keys[d].numpy(), depth, d)
        assert np.array_equal(label, (merged.children[d] >= 0).numpy().astype(np.int64)), d
    rf, ra, rn, S_dot, _ = T.point_features(sk, si, pts, nrm, merged.keys[depth].numpy(), depth)
    # the oracle is fp32 torch with scatter_add in another order: a few units
    assert_close(feat[:, :3], torch.tensor(rf[:, :3]), torch.tensor(np.abs(rf[:, :3])) + 1e-6, 32.0, 'normal')
    assert_close(feat[:, 3], torch.tensor(rf[:, 3]), torch.tensor(S_dot) + 1e-6, 64.0, 'dot')
    assert np.all(rf[merged.children[depth].numpy() < 0] == 0)


def test_points_keys_clamp_and_order():
    one_below = np.nextafter(np.float32(1), np.float32(0))
    pts = np.array([[-1, -1, -1], [one_below] * 3, [1, 1, 1], [-1.5, 0, 1.5], [0, 0, 0]], dtype=np.float32)
    for depth in (1, 6, 16):
        k = T.points_keys(pts, 5, depth)
        hi = 8 ** depth - 1
        assert (k >> 48).tolist() == [5] * 5
        m = k & (2 ** 48 - 1)
        assert m[0] == 0 and m[1] == hi and m[2] == hi and m[4] == 7 * 8 ** (depth - 1)
        assert m[3] == T.morton([0], [2 ** (depth - 1)], [2 ** depth - 1])[0]
    assert T.morton([1], [0], [0])[0] == 4 and T.morton([0], [1], [0])[0] == 2 and T.morton([0], [0], [2])[0] == 8
    keys = np.array([3, 1, 3, 1, 2], dtype=np.int64)
    assert T.points_sort(keys, np.array([9, 8, 7, 6, 5]))[1].tolist() == [8, 6, 5, 9, 7]


def test_point_features_float32_within_the_device_bounds():
    """the inputs of the device test: exact fp32 sums, and the float32 evaluation inside the bounds"""
    g = np.random.default_rng(0)
    cells = np.array([[15, 7, 11], [60, 3, 33]])
    pts = np.concatenate([cells[0] + g.integers(1, 1024, size=(1000, 3)) / 1024.0,
                          cells[1] + g.integers(1, 1024, size=(2, 3)) / 1024.0]) / 32.0 - 1.0
    nrm = g.integers(-1024, 1025, size=(1002, 3)) / 1024.0
    nrm[1001] = -nrm[1000]
    pts, nrm = pts.astype(np.float32), nrm.astype(np.float32)
    sk, si = T.points_sort(T.points_keys(pts, 0, 6), np.arange(1002))
    nodes = np.array([T.morton(*[[c] for c in cells[1]])[0], 5, T.morton(*[[c] for c in cells[0]])[0]], dtype=np.int64)
    rf, ra, rn, S, exact = T.point_features(sk, si, pts, nrm, nodes, 6)
    f32 = T.point_features(sk, si, pts, nrm, nodes, 6, np.float32)
    assert exact and f32[4]
    assert np.all(rf[0] == 0) and np.all(rf[1] == 0) and np.all(ra[1] == 0) and np.all(ra[0] > 0)
    assert_close(torch.tensor(f32[1]), torch.tensor(ra), np.abs(ra), T.POINTS_C_AVG, 'avg_points')
    assert_close(torch.tensor(f32[2]), torch.tensor(rn), np.abs(rn), T.POINTS_C_NORMAL, 'normal')
    assert_close(torch.tensor(f32[0][:, 3]), torch.tensor(rf[:, 3]), S, T.POINTS_C_DOT, 'dot')


# ------------------------------------------------------------------------------------------------ float32 inside the bounds
@pytest.mark.parametrize('kind', ['mix'] + T.CE_BANDS)
def test_cross_entropy_float32_within_the_device_bounds(kind):
    logits, child = T.ce_case_rows(kind, 65537, 11)
    ce, _ = T.ce_rows(logits, child)
    ce32, _ = T.ce_rows(logits, child, np.float32)
    ref = float(ce.sum())
    bound, host, signed = T.ce_loss_bound(logits, child, ref)
    assert abs(float(ce32.astype(np.float64).sum()) - ref) <= bound / 3 and bound <= 3.1 * 3 * U * ref
    want, S, c = T.ce_grad(logits, child, 0.37)
    got, _, _ = T.ce_grad(logits, child, 0.37, np.float32)
    assert np.array_equal(got[:, 0], -got[:, 1])
    assert_close(torch.tensor(got), torch.tensor(want), S, torch.tensor(c), 'dlogits')


def test_confident_logit_table():
    """4096 correctly classified rows +-a per band: the softplus form in fp32 stays inside the device bound in all
    three; m + log(e0 + e1) - l_label loses 1.5e-3 of the loss at a in 4..8 and all of it at a in 8..16."""
    rel_old, rel_new = [], []
    for band in T.CE_BANDS:
        logits, child = T.ce_case_rows(band, 4096, 1)
        assert T.ce_hits(logits, child) == 4096
        ce, _ = T.ce_rows(logits, child)
        ref = float(ce.sum())
        bound, _, _ = T.ce_loss_bound(logits, child, ref)
        new = float(T.ce_rows(logits, child, np.float32)[0].astype(np.float64).sum())
        old = float(T.ce_rows_lse(logits, child).astype(np.float64).sum())
        rel_old.append(abs(old - ref) / ref)
        rel_new.append(abs(new - ref) / ref)
        print('a in %r: softplus fp32 %.1e, m + log(e0 + e1) - l %.1e, bound %.1e (relative)' % (band, rel_new[-1], rel_old[-1],
                                                                                              bound / ref))
        assert abs(new - ref) <= bound
        assert (abs(old - ref) <= bound) == (band == T.CE_BANDS[0])
    assert max(rel_new) < 2e-8 and 1e-3 < rel_old[1] < 2e-3 and rel_old[2] == 1.0


@pytest.mark.parametrize('E', [1, 3, 8])
def test_posterior_float32_within_the_device_bounds(E):
    params, noise, dz = T.posterior_case(4001, E, E)
    (z, S_z), (kl, S_kl) = T.posterior(params, noise, E)
    (z32, _), (kl32, _) = T.posterior(params, noise, E, np.float32)
    assert_close(torch.tensor(z32), torch.tensor(z), S_z, T.KL_C_Z, 'z')
    assert_close(torch.tensor(kl32), torch.tensor(kl), S_kl, T.KL_C_TERM, 'kl')
    assert np.array_equal(T.posterior(params, None, E, np.float32)[0][0], params[:, :E])
    (dm, S_m), (dl, S_l) = T.posterior_bwd(params, noise, dz, E, 0.1)
    (dm32, _), (dl32, _) = T.posterior_bwd(params, noise, dz, E, 0.1, np.float32)
    assert_close(torch.tensor(dm32), torch.tensor(dm), S_m, T.KL_C_DMEAN, 'dmean')
    assert_close(torch.tensor(dl32), torch.tensor(dl), S_l, T.KL_C_DLV, 'dlogvar')


# ------------------------------------------------------------------------------------------------ GroupNorm backward
class _Doctree:
    def __init__(self, bid, B):
        self.bid, self.batch_size = bid.long(), B

    def batch_id(self, depth):
        return self.bid


@pytest.mark.parametrize('C,groups', [(16, 4), (96, 32), (60, 30)])
@pytest.mark.parametrize('act', [None, 'silu', 'gelu'])
def test_gn_backward_equals_the_oracle(C, groups, act):
    """autograd through oracle/modules.dual_octree_group_norm.  It keeps 1 / (count + eps) and eps as doubles; here eps
    is the fp32 value the C ABI carries and the reciprocal is rounded to fp32 as gn_oracle.finalize states it: U relative
    on the mean and the variance.  The mean moves by U |mean|, the normalised value by U |mean| / sigma, and dx answers
    with (1 + |normalised x|) <= 6 times that of S: c = 2 + 6 |mean| / sigma."""
    import glue_oracle as G
    from oracle import modules as OM
    sizes = (40, 0, 7, 1, 23)
    x, dy, bid = T.gn_bwd_inputs(sizes, C, groups, C)
    w, b = GN.make_affine(C, C)
    assert OM.gn_groups(C) == groups
    with torch.enable_grad():
        xd = x.double().requires_grad_(True)
        wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
        y = G.act(OM.dual_octree_group_norm(xd, _Doctree(bid, len(sizes)), 5, wd, bd), act)[0]
        (y * dy.double()).sum().backward()
    ref = T.gn_backward(x, dy, bid, sizes, C, groups, w, b, act)
    c = 2.0 + 6.0 * T.gn_conditioning(x, bid, sizes, C, groups)
    assert c <= 50
    assert_close(ref['dx'], xd.grad, ref['S_dx'], c, 'dx')
    assert_close(ref['dgamma'], wd.grad, ref['S_dgamma'], c, 'dgamma')
    assert_close(ref['dbeta'], bd.grad, ref['S_dbeta'], c, 'dbeta')
    # S is what it says: the three parts add up to dx
    lead = w.double() * ref['r'][bid.long()] * ref['g']
    assert float((ref['S_dx'] - (ref['dx'] - lead).abs() - lead.abs()).min()) >= -1e-12 * float(ref['S_dx'].max())


def test_stats_rows_is_the_kernels_rule():
    """the by-hand figures of gn_oracle.STATS_BIG, and the two large cases of the device test"""
    for C, n, rows in GN.STATS_BIG:
        assert T.stats_rows(n, 1, C) == rows
    assert T.stats_rows(4100, 1) == 128 and T.stats_rows(8200, 1) == 192 and T.stats_rows(393, 6) == 64
    assert 8200 * (1024 // 4) > T.GRID_CAP


def _gn_case(C, groups, sizes, count_eps):
    seed = T.gn_seed(C, groups, sizes)
    x, dy, bid = T.gn_bwd_inputs(sizes, C, groups, seed)
    w, b = GN.make_affine(C, seed)
    return x, dy, bid, w, b


@pytest.mark.parametrize('rows', ['ragged', 'seventy'])
@pytest.mark.parametrize('C,groups', T.GN_WIDTHS)
def test_gn_backward_inputs_and_host_ratios(C, groups, rows):
    """the inputs of the device test are conditioned as it asserts; the worst ratio of the float32 host evaluation stays
    under the figures recorded in train_oracle.GN_HOST_RATIOS (3 x the measured one is the device bound)"""
    sizes = T.gn_sizes(C, groups, rows)
    x, dy, bid, w, b = _gn_case(C, groups, sizes, GN.EPS)
    assert T.gn_conditioning(x, bid, sizes, C, groups) <= 8.0
    for act in GN.ACT_ID:
        ref = T.gn_backward(x, dy, bid, sizes, C, groups, w, b, act)
        c_dx, c_dg, c_db, ratios = T.gn_c(ref, x, dy, bid, sizes, C, groups, w, b, act)
        print('C %d groups %d %s %s: host ratios dx %.1f dgamma %.1f dbeta %.1f' % (C, groups, rows, act, *ratios))
        for r, cap in zip(ratios, T.GN_HOST_RATIOS):
            assert r <= cap
        assert c_dx >= T.GN_C_FLOOR and c_dx == max(T.GN_C_FLOOR, 3 * ratios[0])


@pytest.mark.parametrize('C,groups', T.GN_COUNT_EPS_WIDTHS)
def test_gn_backward_count_eps_terms_matter(C, groups):
    """count_eps = 0.5 on elements of 1 to 3 rows: a backward without the count_eps terms misses the device bound by
    more than four orders of magnitude, the float32 evaluation with them stays inside it"""
    sizes = T.GN_COUNT_EPS_SIZES
    x, dy, bid, w, b = _gn_case(C, groups, sizes, 0.5)
    assert T.gn_conditioning(x, bid, sizes, C, groups, count_eps=0.5) <= 8.0
    for act in GN.ACT_ID:
        ref = T.gn_backward(x, dy, bid, sizes, C, groups, w, b, act, count_eps=0.5)
        c_dx, _, _, ratios = T.gn_c(ref, x, dy, bid, sizes, C, groups, w, b, act, count_eps=0.5)
        without = T.gn_backward(x, dy, bid, sizes, C, groups, w, b, act, count_eps=0.5, drop_count_eps_terms=True)
        miss = float(((without['dx'] - ref['dx']).abs() / (c_dx * U * ref['S_dx'])).max())
        print('C %d groups %d %s: c %.1f, without the count_eps terms %.3g times the bound' % (C, groups, act, c_dx, miss))
        assert miss > 1e4 and c_dx <= 3 * 20
