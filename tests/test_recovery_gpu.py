# -*- coding: utf-8 -*-
'''
Gradient recovery and the ZZ indicator on the HIP path (flow_amd/fem/
recovery.py; csrc/recovery_kernels.hip) against the numpy restatement of
tests/recovery_reference.py.

The bound.  max |G_gpu - G_ref| <= 1e-12 * max |G_ref| and max |eta2_gpu -
eta2_ref| <= 1e-12 * max eta2_ref: a patch sum has at most eight terms per
sum with weights of one sign, a cell integral at most nine points of up to
24 squares, the two sides add them in different orders (the kernel in the
order of the contribution map, the restatement by ascending cell; two
different exact quadrature rules).  That is rounding, a few hundred ulps,
with two orders of margin for G.  eta2 is a sum of squares of the DIFFERENCE
G - grad u, so its relative rounding is about 1e-15 |G| / |G - grad u|; the
fields (recovery_reference.smooth0 / smooth1) oscillate enough that the
difference is at least 2e-2 |G| where eta2 is largest on every mesh and
degree here: two numpy evaluations of the formula with different exact rules
then agree to 2e-14 of max eta2 or better.

Meshes and fields: recovery_reference.mesh / smooth0 / smooth1 (see there).
Every test prints its measured error next to its bound (pytest -s).
'''
import functools

import numpy
import pytest
import torch

from flow_amd import device, fem
from flow_amd.fem import GradientRecovery

import recovery_reference as rref

pytestmark = pytest.mark.gpu

TOL = 1e-12


@functools.lru_cache(maxsize=None)
def _case(name, deg, dim):
    '''(u, reference G (dim, 2, N), reference eta2) of the interpolated
    smooth fields, computed once.'''
    V = fem.FunctionSpace(rref.mesh(name), 'CG', deg, dim=dim)
    u = rref.field(V, [rref.smooth0, rref.smooth1][:dim])
    G = rref.gradient(u)
    eta2 = rref.indicator(u, G)
    G.flags.writeable = False
    eta2.flags.writeable = False
    return u, G, eta2


def _host(G, dim):
    '''What apply() returned as (dim, 2, N).'''
    fs = [G] if dim == 1 else list(G)
    return numpy.array([f.array().reshape(2, -1) for f in fs])


def _close(got, want, what):
    scale = numpy.abs(want).max()
    err = numpy.abs(got - want).max()
    print('%s: error %.2e  bound %.2e' % (what, err, TOL * scale))
    assert numpy.isfinite(got).all()
    assert err <= TOL * scale


# -- 1. against the restatement ------------------------------------------------------
@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('name', rref.MESHES)
def test_against_reference(hip, name, deg, dim):
    u, Gref, eref = _case(name, deg, dim)
    V = u.function_space()
    R = GradientRecovery(V)
    G = R.apply(u)
    for f in ([G] if dim == 1 else G):
        assert isinstance(f, fem.Function)
        assert f.function_space().same_as(
            fem.VectorFunctionSpace(V.mesh(), 'CG', deg))
    if dim == 2:
        assert isinstance(G, tuple) and len(G) == 2
    _close(_host(G, dim), Gref, '%s P%d x%d G' % (name, deg, dim))
    eta2 = R.indicator(u)
    assert eta2.dtype == torch.float64 and eta2.is_cuda
    assert tuple(eta2.shape) == (V.mesh().num_cells(),)
    _close(device.to_host(eta2).numpy(), eref,
           '%s P%d x%d eta2' % (name, deg, dim))


# -- 2. exactness ----------------------------------------------------------------------
@pytest.mark.parametrize('deg,dim', [(1, 1), (2, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize('name', rref.MESHES)
def test_polynomials_of_the_degree_are_recovered_exactly(hip, name, deg, dim):
    '''A linear field on P1 gives its constant gradient, a quadratic field on
    P2 its linear gradient, at EVERY node (one-sided patches included), and
    eta2 vanishes to rounding: a wrong mid-point position or weight that a
    like-minded restatement might share does not pass here.'''
    mesh = rref.mesh(name)
    V = fem.FunctionSpace(mesh, 'CG', deg, dim=dim)
    funcs, grads, gmax = rref.EXACT[(deg, dim)]
    u = rref.field(V, funcs)
    R = GradientRecovery(V)
    got = _host(R.apply(u), dim)
    xy = V.layout.dof_coords
    want = numpy.array([numpy.broadcast_arrays(*g(xy[:, 0], xy[:, 1]))
                        for g in grads])
    err = numpy.abs(got - want).max()
    eta2 = device.to_host(R.indicator(u)).numpy()
    bound = 1e-22 * gmax**2 * numpy.abs(mesh.cell_areas()).sum()
    print('%s P%d x%d: gradient error %.2e (1e-12), eta2 max %.2e (%.2e)'
          % (name, deg, dim, err, eta2.max(), bound))
    assert err <= 1e-12
    assert numpy.isfinite(eta2).all() and eta2.min() >= 0.0
    assert eta2.max() <= bound


# -- 3. determinism and out= -----------------------------------------------------------
@pytest.mark.parametrize('dim', [1, 2])
def test_same_bits_twice_and_out(hip, dim):
    u, Gref, eref = _case('square 24', 2, dim)
    V = u.function_space()
    R = GradientRecovery(V)
    a, b = R.apply(u), R.apply(u)
    fa = [a] if dim == 1 else list(a)
    fb = [b] if dim == 1 else list(b)
    for x, y in zip(fa, fb):
        assert x.data.data_ptr() != y.data.data_ptr()
        assert torch.equal(x.data, y.data)
    # into existing Functions: separately allocated ones, ...
    sep = [fem.Function(R.G) for _ in range(dim)]
    for f in sep:
        f.data.fill_(-1.0)
    out = sep[0] if dim == 1 else tuple(sep)
    assert R.apply(u, out=out) is out
    for x, y in zip(fa, sep):
        assert torch.equal(x.data, y.data)
    # ... and the ones apply() handed out (one buffer)
    for f in fb:
        f.data.fill_(-1.0)
    assert R.apply(u, out=b) is b
    for x, y in zip(fa, fb):
        assert torch.equal(x.data, y.data)
    e1, e2 = R.indicator(u), R.indicator(u)
    assert e1.data_ptr() != e2.data_ptr() and torch.equal(e1, e2)
    buf = device.empty(len(eref))
    buf.fill_(-1.0)
    assert R.indicator(u, out=buf) is buf and torch.equal(buf, e1)
    with pytest.raises(ValueError, match='out'):
        R.indicator(u, out=device.empty(len(eref) + 1))
    est = R.estimate(u)
    ref = float(numpy.sqrt(eref.sum()))
    print('estimate %.15e reference %.15e' % (est, ref))
    assert isinstance(est, float) and abs(est - ref) <= 1e-12 * ref
    # the one-off spellings
    one = fem.recover_gradient(u)
    for x, y in zip(fa, [one] if dim == 1 else list(one)):
        assert torch.equal(x.data, y.data)
    assert torch.equal(fem.zz_indicator(u), e1)


# -- 4. a vector field is its components --------------------------------------------------
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('name', ['hole refined', 'square 24'])
def test_vector_rows_equal_scalar_recoveries_bitwise(hip, name, deg):
    w, _, _ = _case(name, deg, 2)
    W = w.function_space()
    G0, G1 = GradientRecovery(W).apply(w)
    R = GradientRecovery(W.collapse())
    for comp, G in zip(w.split(), (G0, G1)):
        assert torch.equal(R.apply(comp).data, G.data)


# -- 5. downstream ----------------------------------------------------------------------
def test_indicator_feeds_mark_and_probes_take_the_gradient(hip):
    u, _, eref = _case('fitted hole', 1, 1)
    R = GradientRecovery(u.function_space())
    mask = fem.mark(R.indicator(u), 0.5)
    assert isinstance(mask, numpy.ndarray) and mask.dtype == bool
    assert mask.shape == (len(eref),) and 0 < mask.sum() < len(eref)
    # the recovered gradient of a quadratic on P2 is its linear gradient:
    # Probes interpolate it exactly between the nodes too
    mesh = rref.mesh('fitted hole')
    V = fem.FunctionSpace(mesh, 'CG', 2)
    G = fem.recover_gradient(rref.field(V, [rref.quadratic]))
    pts = numpy.array([[0.03, 0.02], [0.71, 0.33], [0.25, 0.41], [0.97, 0.07]])
    got = fem.Probes(mesh, pts)(G)
    want = numpy.stack(rref.quadratic_grad(pts[:, 0], pts[:, 1]), axis=1)
    print('probes: error %.2e' % numpy.abs(got - want).max())
    assert got.shape == (4, 2) and numpy.abs(got - want).max() <= 1e-12


# -- 6. superconvergence ------------------------------------------------------------------
def test_recovered_gradient_is_superconvergent(hip):
    '''u = sin(pi x) sin(pi y), P1 interpolant, UnitSquareMesh(8, 8) and
    (16, 16): the recovered gradient is nearer to grad u than the cell
    gradient on both meshes and falls by a larger factor between them (the
    restatement: 3.06 against 1.99, tests/test_recovery_host.py).  Norms by
    forms on the device, the exact gradient evaluated at the rule's points.'''
    from flow_amd.fem import SpatialCoordinate, as_vector, assemble, cos, dx, \
        grad, inner, sin
    rows = []
    for n in (8, 16):
        mesh = fem.UnitSquareMesh(n, n)
        u = rref.field(fem.FunctionSpace(mesh, 'CG', 1), [rref.bubble])
        G = fem.recover_gradient(u)
        X = SpatialCoordinate(mesh)
        ge = as_vector([fem.pi * cos(fem.pi * X[0]) * sin(fem.pi * X[1]),
                        fem.pi * sin(fem.pi * X[0]) * cos(fem.pi * X[1])])
        par = {'quadrature_degree': 6}
        rec = numpy.sqrt(assemble(inner(G - ge, G - ge) * dx, par))
        raw = numpy.sqrt(assemble(inner(grad(u) - ge, grad(u) - ge) * dx, par))
        rows.append((rec, raw))
    print('recovered %.4e -> %.4e (x %.2f), raw %.4e -> %.4e (x %.2f)'
          % (rows[0][0], rows[1][0], rows[0][0] / rows[1][0],
             rows[0][1], rows[1][1], rows[0][1] / rows[1][1]))
    for rec, raw in rows:
        assert rec < raw
    assert rows[0][0] / rows[1][0] > rows[0][1] / rows[1][1]
