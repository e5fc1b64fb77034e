"""tests/mpu_oracle.py on the host: the float64 restatement of the NeuralMPU agrees with oracle/mpu.py (float32) and with
the reference's own outputs (tests/golden/g_mpu.pt) inside the bounds the GPU tests use, its gradient and adjoint agree
with float64 autograd through a second statement of the formulas kept here, and the bounds reject five planted errors.
"""
import functools

import numpy as np
import pytest
import torch

import graph_oracle as G
import mpu_oracle as M

TREES = ('deep_a', 'deep_b_mid', 'deep_c', 'full_face')
RANGE_IDS = ('fd..depth', 'fd..fd', 'fd+1..depth', 'depth..depth', '0..fd+1')


@functools.lru_cache(maxsize=None)
def key_tree(name):
    return M.KeyTree(G.tree(name)[0])


@functools.lru_cache(maxsize=None)
def case(name, ri, n=4099):
    """(T, ds, de, pts, kind, code, dsdf, dgrad, R): one tree, one depth range, n generated points, evaluated once."""
    T = key_tree(name)
    ds, de = M.ranges(T)[ri]
    pts, kind = M.points(T, ds, de, n, seed=TREES.index(name))
    code = M.code_table(T, ds, de, seed=ri)
    g = np.random.default_rng(99 + ri)
    dsdf = g.standard_normal(n).astype(np.float32)
    dgrad = g.standard_normal((n, 3)).astype(np.float32)
    R = M.evaluate(T, ds, de, pts, code, dsdf, dgrad)
    return T, ds, de, pts, kind, code, dsdf, dgrad, R


def ratios(got, R, nd):
    """worst |got - ref| / bound of (sdf, grad, dcode); 0 / 0 counts as 0, x / 0 as inf"""
    out = []
    for key, bound in zip(('sdf', 'grad', 'dcode'), M.bounds(R, nd)):
        if got.get(key) is None:
            out.append(0.0)
            continue
        err = np.abs(np.asarray(got[key], dtype=np.float64) - R[key])
        with np.errstate(divide='ignore', invalid='ignore'):
            q = np.where(err == 0, 0.0, err / bound)
        out.append(float(q.max()) if q.size else 0.0)
    return out


@torch.enable_grad()
def oracle32(name, ds, de, pts, code, dsdf, dgrad):
    """oracle/mpu.py in float32; grad and dcode by float32 autograd through it"""
    from oracle import mpu as OMPU
    oc = G.tree(name)[0]
    p = torch.tensor(pts).requires_grad_(True)
    c = torch.tensor(code).requires_grad_(True)
    sdf, mask = OMPU.linear_pred(p, oc, c, ds, de)
    grad, = torch.autograd.grad(sdf.sum(), p, create_graph=True)
    grad = grad[:, :3]
    loss = (sdf * torch.tensor(dsdf)).sum() + (grad * torch.tensor(dgrad)).sum()
    dcode, = torch.autograd.grad(loss, c)
    return dict(sdf=sdf.detach().numpy(), mask=mask.numpy(), grad=grad.detach().numpy(), dcode=dcode.numpy())


# ------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize('name', TREES)
def test_points_cover_what_they_promise(name):
    T = key_tree(name)
    for ri, (ds, de) in enumerate(M.ranges(T)):
        for n in M.COUNTS:
            pts, kind = M.points(T, ds, de, n, seed=TREES.index(name))
            assert pts.dtype == np.float32 and pts.shape == (n, 4) and np.isfinite(pts).all()
            R = M.evaluate(T, ds, de, pts, M.code_table(T, ds, de))
            assert 2 * int(R['mask'].sum()) >= n, (ds, de, n)
        _, _, _, pts, kind, _, _, _, R = case(name, ri)
        B = T.batch_size
        want_kinds = set(range(10)) - (set() if M.empty_elements(T) else {7}) - ({6, 7} if de <= T.full_depth else set())
        assert set(kind.tolist()) == want_kinds
        b = M.batch_of(pts)
        assert {-1, B, B + 3} <= set(b.tolist())
        assert np.any(pts[:, 3] == np.float32(0.5)) and np.any(pts[:, 3] == np.float32(B - 0.001))
        assert np.all(b[pts[:, 3] == np.float32(B - 0.001)] == B - 1)
        out = (b < 0) | (b >= B)
        assert not R['mask'][out].any() and np.all(R['used'][out] == 0)
        assert not R['mask'][kind == 6].any() and not R['mask'][kind == 7].any()
        # on a centre plane / on a face of every depth of the range, and on / outside the cube
        for d in range(ds, de + 1):
            X = M.cell_coord(pts[:, :3], d)
            assert np.any((X == np.floor(X)) & (kind == 2)[:, None]), ('no centre plane of depth', d)
            assert np.any((X + 0.5 == np.floor(X + 0.5)) & (kind == 3)[:, None]), ('no face of depth', d)
        assert np.any(np.abs(pts[kind == 4, :3]) == 1.0) and np.any(np.abs(pts[kind == 5, :3]) > 1.0)
        # a centre that is used sits exactly on a plane somewhere: the one place sgn(0) matters
        hit = False
        for d in range(ds, de + 1):
            _, _, use, f = M.visit(T, d, de, pts, None)
            hit |= bool(np.any((f == 0).any(-1) & use))
        assert hit, 'no used centre with an offset of exactly 0'


# ------------------------------------------------------------------------------------------------ agreement
@pytest.mark.parametrize('ri', range(5), ids=RANGE_IDS)
@pytest.mark.parametrize('name', TREES)
def test_float32_oracle_inside_the_bounds(name, ri):
    T, ds, de, pts, kind, code, dsdf, dgrad, R = case(name, ri)
    got = oracle32(name, ds, de, pts, code, dsdf, dgrad)
    assert np.array_equal(got['mask'], R['mask'])
    r = ratios(got, R, de - ds + 1)
    print('float32 oracle / bound %s %d..%d: sdf %.3f grad %.3f dcode %.3f' % ((name, ds, de) + tuple(r)))
    assert max(r) <= 1.0, r


def test_golden_reference_outputs(golden):
    """the reference's own mpu.py outputs sit inside the sdf bound of the float64 restatement"""
    from test_oracle_golden import mpu_case
    Gd = golden('g_mpu')
    oc_l, reg, (fd, ds, dp) = mpu_case(Gd)
    T = M.KeyTree(oc_l)
    pts = Gd['pos'].numpy().astype(np.float32)
    for d in range(ds, dp + 1):
        R = M.evaluate(T, fd, d, pts, reg[d].numpy())
        assert np.array_equal(R['mask'], Gd['mask'][d].numpy().astype(bool))
        r = ratios(dict(sdf=Gd['sdf'][d].numpy()), R, d - fd + 1)
        assert r[0] <= 1.0, (d, r)
        assert int(R['mask'].sum()) > 0


# ------------------------------------------------------------------------------------------------ gradient and adjoint
@torch.enable_grad()
def torch_mpu(T, ds, de, pts, code):
    """A second float64 statement, differentiable: (sdf, grad) as torch tensors, grad by autograd w.r.t. the position
    with the floor detached and d|f|/df = +1 at 0.  The position enters as the float32 cell coordinate plus a zero that
    carries the derivative 2^(d-1)."""
    p = torch.tensor(pts[:, :3].astype(np.float64), requires_grad=True)
    num = torch.zeros(pts.shape[0], dtype=torch.float64)
    den = torch.zeros_like(num)
    base = 0
    for d in range(ds, de + 1):
        idx, found, use, _ = M.visit(T, d, de, pts)
        X = torch.tensor(M.cell_coord(pts[:, :3], d)) + (p - p.detach()) * 2.0 ** (d - 1)
        centre = torch.floor(X.detach()).unsqueeze(1) + torch.tensor(M.CORNERS, dtype=torch.float64)
        f = X.unsqueeze(1) - centre
        absf = torch.where(f < 0, -f, f)
        w = (1.0 - absf).prod(-1) * float(np.float32(d * d / 50.0))
        c = code[torch.tensor(np.where(use, idx + base, 0))]
        val = (c[..., :3] * f * (2.0 / 2 ** d)).sum(-1) + c[..., 3]
        u = torch.tensor(use)
        num = num + torch.where(u, w * val, torch.zeros_like(w)).sum(-1)
        den = den + torch.where(u, w, torch.zeros_like(w)).sum(-1)
        base += T.nnum[d]
    sdf = num / (den + M.EPS)
    grad, = torch.autograd.grad(sdf.sum(), p, create_graph=True)
    return sdf, grad


@pytest.mark.parametrize('ri', range(5), ids=RANGE_IDS)
@pytest.mark.parametrize('name', TREES)
def test_gradient_and_adjoint(name, ri):
    T, ds, de, pts, kind, code, dsdf, dgrad, R = case(name, ri)
    c = torch.tensor(code.astype(np.float64), requires_grad=True)
    sdf, grad = torch_mpu(T, ds, de, pts, c)
    with torch.enable_grad():
        loss = (sdf * torch.tensor(dsdf.astype(np.float64))).sum() + (grad * torch.tensor(dgrad.astype(np.float64))).sum()
    with torch.enable_grad():
        dcode, = torch.autograd.grad(loss, c)
    tiny = 1e-12                                       # float64 against float64: a thousand roundings of 2^-53
    assert np.abs(sdf.detach().numpy() - R['sdf']).max() <= tiny * max(1.0, np.abs(R['S'] / R['D']).max())
    assert np.all(np.abs(grad.detach().numpy() - R['grad']) <= tiny * np.maximum(R['gabs'], 1.0))
    assert np.all(np.abs(dcode.numpy() - R['dcode']) <= tiny * np.maximum(R['dabs'], 1.0))
    # <dcode, c'> = <dsdf, sdf(c')> + <dgrad, grad(c')>: both outputs are linear in the code
    c2 = np.random.default_rng(5).standard_normal(code.shape)
    R2 = M.evaluate(T, ds, de, pts, c2)
    lhs = float((R['dcode'] * c2).sum())
    rhs = float((dsdf * R2['sdf']).sum() + (dgrad * R2['grad']).sum())
    scale = float((R['dabs'] * np.abs(c2)).sum())
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs, scale)
    # accumulation into a table that is not zero
    R3 = M.evaluate(T, ds, de, pts, code, dsdf, dgrad, dcode0=c2)
    assert np.allclose(R3['dcode'], R['dcode'] + c2, rtol=0, atol=1e-12 * R3['dabs'].max())
    assert np.all(R3['dabs'] >= R['dabs'])


# ------------------------------------------------------------------------------------------------ the bounds have teeth
# the ranges (indices into mpu_oracle.ranges) on which each planted error changes the function.  Where a single depth
# contributes to a point, k_d cancels from num / den, the leaf rule and the row base do nothing, and so does sgn(0): the
# centres with f_a = 0 are then the only ones with a weight, and sum_i dw_ia (v_i - sdf) over them is 0 by the definition
# of sdf.  The row base moves only past a depth that has leaves.
SHOWS_ON = {'kd_next': (0, 2, 4), 'no_leaf_rule': (0, 2, 4), 'sgn0': (0, 2, 4), 'row_base_nempty': (0, 2, 4),
            'corner_flip': (0, 1, 2, 3, 4)}


@pytest.mark.parametrize('mutant', M.MUTANTS)
@pytest.mark.parametrize('name', TREES)
def test_bounds_reject_planted_errors(name, mutant):
    for ri in SHOWS_ON[mutant]:
        T, ds, de, pts, kind, code, dsdf, dgrad, R = case(name, ri)
        if mutant == 'row_base_nempty' and T.nnum[ds:de] == T.nnum_nempty[ds:de]:
            continue                                   # no leaf above de: the two row bases are the same numbers
        bad = M.evaluate(T, ds, de, pts, code, dsdf, dgrad, mutant=mutant)
        r = ratios(bad, R, de - ds + 1)
        if mutant == 'sgn0' and name == 'full_face' and ds > T.full_depth:
            continue                                   # no leaf between depths 3 and 5: only depth 6 contributes
        assert max(r) > 1.0, (mutant, name, ds, de, r)
        if mutant == 'sgn0':
            assert r[1] > 1.0 and r[2] > 1.0 and r[0] == 0.0, r    # the value does not depend on sgn
