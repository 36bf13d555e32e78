# -*- coding: utf-8 -*-
'''
fem.BoundaryProfile on the HIP path (flow_amd/fem/profile.py,
csrc/form_kernels.hip: form_facet_values_kernel, profile_cumsum_kernel)
against the numpy restatement of tests/profile_reference.py.

Meshes: UnitSquareMesh(3, 2) and rectangle_with_hole(0, 1, 0, 0.5, (0.4,
0.25), 0.12, 18, 9).  (tests/cases.py holds no rectangle_with_hole; of the
staircase meshes of this shape 16 x 8 gives 62 facets, 248 samples at degree
6 (m = 4), one block; 18 x 9 is the next: 73 facets, 292 samples, a full block
and a partial one.)  m = 4 divides the 256 lanes of a block, so a block
boundary can never fall inside a facet's samples at degree 6: the hole mesh
also runs at degree 8 (m = 5, 365 samples, lane 256 is sample 1 of facet 51).

Tolerances: those of the form kernels against their numpy evaluator
("Checks"; tests/test_bilinear_forms_gpu.py): entries < 1e-12 of
the largest entry, integrals < 1e-13.
'''
import ctypes
import functools

import numpy
import pytest
import torch

from flow_amd import fem, karman, device, _hip
from flow_amd.fem import (
    assemble, Measure, FacetNormal, MeshFunction, SpatialCoordinate,
    CellDiameter, conditional, gt, sqrt, dot, inner, grad,
    )

import profile_reference as pref

pytestmark = pytest.mark.gpu

HOLE = (0.0, 1.0, 0.0, 0.5, (0.4, 0.25), 0.12, 18, 9)
MU = 0.3


def _host(t):
    return device.to_host(t).numpy()


class _Hole(fem.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary & (x[0] > 1e-9) & (x[0] < 1.0 - 1e-9) \
            & (x[1] > 1e-9) & (x[1] < 0.5 - 1e-9)


@functools.lru_cache(maxsize=None)
def _case(name):
    '''(mesh, fields) shared by the tests: never modified.'''
    mesh = fem.UnitSquareMesh(3, 2) if name == 'square' \
        else fem.rectangle_with_hole(*HOLE)
    P1 = fem.FunctionSpace(mesh, 'CG', 1)
    P2 = fem.FunctionSpace(mesh, 'CG', 2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    p = fem.interpolate(fem.Expression('exp(x[0])*x[1] + 2', degree=3), P1)
    th = fem.interpolate(fem.Expression('0.5 + x[0]*x[1] + sin(5*x[0])',
                                        degree=3), P2)
    u = fem.Function(W)
    xy = W.layout.dof_coords
    u.set_array(numpy.concatenate([
        numpy.sin(7 * xy[:, 0]) * xy[:, 1] + 1.0,
        numpy.cos(9 * xy[:, 1]) * xy[:, 0] - 0.4]))
    markers = MeshFunction('size_t', mesh, 1, 0)
    _Hole().mark(markers, 5)
    return mesh, dict(p=p, th=th, u=u, markers=markers)


@functools.lru_cache(maxsize=None)
def _pair(name, degree):
    '''(profile, restatement) of the whole boundary.'''
    mesh, _ = _case(name)
    P = fem.BoundaryProfile(mesh, degree=degree)
    R = pref.Reference(mesh, range(len(mesh.bfacets)), degree)
    return P, R


CASES = [('square', 2), ('hole', 6), ('hole', 8)]


def _close(got, want, tol=1e-12):
    got, want = numpy.asarray(got), numpy.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = numpy.abs(got - want).max() / numpy.abs(want).max()
    print('max error / max entry: %.2e' % err)
    assert err < tol, err


def _stress_normal(R, u):
    '''(2, n): (grad u + grad u^T) n at the samples.'''
    g = numpy.stack([R.grad(u, 0), R.grad(u, 1)])       # g[a, b] = d_b u_a
    return numpy.einsum('abn,bn->an', g + g.transpose(1, 0, 2), R.normal)


def test_sizes():
    P, _ = _pair('hole', 6)
    assert P.nfacets == 73 and P.npoints == 292 and P.m == 4
    assert P.facet_flip.any() and not P.facet_flip.all()
    P, _ = _pair('hole', 8)
    assert P.npoints == 365 and 256 % P.m != 0


@pytest.mark.parametrize('name,degree', CASES)
def test_evaluate_against_restatement(hip, name, degree):
    mesh, f = _case(name)
    P, R = _pair(name, degree)
    p, th, u = f['p'], f['th'], f['u']
    n = FacetNormal(mesh)
    X = SpatialCoordinate(mesh)
    # coordinates and normals of every sample, flipped and unflipped facets
    _close(_host(P.evaluate(X)), R.x)
    _close(_host(P.evaluate(X)), P.x, 1e-15)
    _close(_host(P.evaluate(n)), R.normal)
    # fields and their normal derivatives
    _close(_host(P.evaluate(p)), R.field(p)[None])
    _close(_host(P.evaluate(th)), R.field(th)[None])
    _close(_host(P.evaluate(dot(grad(p), n))),
           (R.grad(p) * R.normal).sum(axis=0)[None])
    _close(_host(P.evaluate(dot(grad(th), n))),
           (R.grad(th) * R.normal).sum(axis=0)[None])
    _close(_host(P.evaluate(u)), numpy.stack([R.field(u, 0), R.field(u, 1)]))
    # the builders
    sn = _stress_normal(R, u)
    t = numpy.stack([-R.normal[1], R.normal[0]])
    _close(_host(P.evaluate(fem.wall_shear(u, fem.Constant(MU)))),
           MU * (t * sn).sum(axis=0)[None])
    _close(_host(P.evaluate(fem.traction(u, p, MU))),
           -(MU * sn - R.field(p)[None] * R.normal))
    _close(_host(P.evaluate(fem.pressure_coefficient(p, 2.0, 1.5, 0.3))),
           ((R.field(p) - 2.0) / (0.5 * 1.5 * 0.09))[None])
    _close(_host(P.evaluate(fem.normal_flux(th, 1.0 + 0.1 * th))),
           -((1.0 + 0.1 * R.field(th))
             * (R.grad(th) * R.normal).sum(axis=0))[None])
    # a tensor: two launches
    g = numpy.stack([R.grad(u, 0), R.grad(u, 1)]).reshape(4, -1)
    _close(_host(P.evaluate(grad(u))), g)
    # an Expression operand
    ex = fem.Expression('sin(4*x[0]) + x[1]*x[1]', degree=4)
    _close(_host(P.evaluate(ex * th + X[0])),
           (R.expression(ex) * R.field(th) + R.x[0])[None])
    # an EXT program
    un = (numpy.stack([R.field(u, 0), R.field(u, 1)]) * R.normal).sum(axis=0)
    _close(_host(P.evaluate(conditional(gt(dot(u, n), 0.0), th, -p)
                            * CellDiameter(mesh))),
           (numpy.where(un > 0.0, R.field(th), -R.field(p)) * R.diameter())[None])


@pytest.mark.parametrize('name,degree', CASES[:2])
def test_linear_field_has_the_one_sided_trace(hip, name, degree):
    mesh, _ = _case(name)
    P, R = _pair(name, degree)
    n = FacetNormal(mesh)
    a, b = 0.25, numpy.array([0.7, -1.3])
    want = (b[:, None] * R.normal).sum(axis=0)[None]
    for deg in (1, 2):
        V = fem.FunctionSpace(mesh, 'CG', deg)
        u = fem.Function(V)
        xy = V.layout.dof_coords
        u.set_array(a + xy.dot(b))
        _close(_host(P.evaluate(dot(grad(u), n))), want, 1e-13)


@pytest.mark.parametrize('name,degree', CASES)
def test_integrate_cumulative_total(hip, name, degree):
    mesh, f = _case(name)
    P, R = _pair(name, degree)
    p, th, u = f['p'], f['th'], f['u']
    n = FacetNormal(mesh)
    flux = dot(grad(th), n) * p
    want = R.facet_sums(numpy.stack([
        R.field(u, 0) * R.field(th), R.field(u, 1) * R.field(th)]))
    parts = _host(P.integrate(u * th))
    _close(parts, want, 1e-13)
    _close(_host(P.integrate(flux)), R.facet_sums(
        ((R.grad(th) * R.normal).sum(axis=0) * R.field(p))[None]), 1e-13)
    # the running sums: numpy.cumsum per curve, bit for bit
    run = _host(P.cumulative(u * th))
    tot = _host(P.total(u * th))
    assert run.shape == parts.shape and tot.shape == (2, P.num_curves)
    for c in range(P.num_curves):
        lo, hi = P.curve_facets[c], P.curve_facets[c + 1]
        for o in range(2):
            assert numpy.array_equal(run[o, lo:hi], numpy.cumsum(parts[o, lo:hi]))
            assert tot[o, c] == run[o, hi - 1]
    # the sum over the facets against assemble at the same degree
    f0 = sqrt(inner(u, u) + 1.0) * th + dot(grad(p), n)**2
    whole = assemble(f0 * Measure('ds', domain=mesh)(degree=degree))
    got = float(_host(P.total(f0)).sum())
    print('whole boundary: %.17g %.17g' % (got, whole))
    assert abs(got - whole) < 1e-13 * abs(whole)
    if name == 'hole':
        dsm = Measure('ds', domain=mesh, subdomain_data=f['markers'])
        part = assemble(f0 * dsm(5, degree=degree))
        Q = fem.BoundaryProfile(mesh, (f['markers'], 5), degree=degree)
        assert Q.num_curves == 1 and Q.closed[0]
        assert Q.nfacets == P.curve_facets[2] - P.curve_facets[1]
        got = float(_host(Q.total(f0))[0, 0])
        print('hole: %.17g %.17g' % (got, part))
        assert abs(got - part) < 1e-13 * abs(part)
        # a SubDomain selects the same curve: the same bits
        S = fem.BoundaryProfile(mesh, _Hole(), degree=degree)
        assert torch.equal(S.evaluate(f0), Q.evaluate(f0))


def test_integrals_have_the_bits_of_the_facet_functional(hip):
    from flow_amd.fem import forms, ops
    mesh, f = _case('hole')
    P, _ = _pair('hole', 6)
    n = FacetNormal(mesh)
    f0 = sqrt(inner(f['u'], f['u']) + 1.0) * f['th'] + dot(grad(f['p']), n)
    prog = forms.compile_trees([forms.as_form(f0).comps], facet=True)
    fs, keep = ops._form_struct(prog, mesh, 6, True)
    cells, local, nf = ops.facet_lists(mesh)
    scratch = device.empty(nf)
    res = ctypes.c_double(0.0)
    _hip.check(hip.flow_form_facet_functional(
        ctypes.byref(ops.mesh_struct(mesh)), ctypes.byref(fs), nf,
        _hip.i32(cells, nf), _hip.i32(local, nf), _hip.f64(scratch, nf),
        _hip.f64(ops.work(_hip.REDUCE_WORK)), ctypes.byref(res), _hip.stream()))
    per_facet = _host(scratch)                  # boundary-facet order
    got = _host(P.integrate(f0))[0]
    assert numpy.array_equal(got, per_facet[P.facet_index])


def test_forces_of_the_karman_case(hip):
    '''integrate(traction) summed over the obstacle against forces() of the
    Karman case of tests/test_facet_forms_gpu.py.'''
    problem = karman.KarmanProblem(60, 14)
    problem.set_initial_stokes()
    want = problem.forces()
    expr = fem.traction(problem.u0, problem.p0, problem.mu)
    # forces() integrates at the degree assemble estimates
    q = fem.forms.check_degree(
        (fem.forms.as_form(expr)[0] * fem.ds(problem.mesh)).degree())
    P = fem.BoundaryProfile(problem.mesh,
                            karman.ObstacleBoundary(problem.length), degree=q)
    assert P.num_curves == 1 and P.closed[0] and P.nfacets >= 8
    parts = _host(P.integrate(expr))
    drag, lift = float(parts[0].sum()), float(parts[1].sum())
    print('drag %.17g %.17g  lift %.17g %.17g'
          % (drag, want['drag'], lift, want['lift']))
    assert abs(drag - want['drag']) < 1e-12 * abs(want['drag'])
    assert abs(lift - want['lift']) < 1e-12 * abs(want['lift'])
    tot = _host(P.total(expr))
    assert abs(tot[0, 0] - want['drag']) < 1e-12 * abs(want['drag'])


def test_determinism_out_uploads_and_empty(hip, monkeypatch):
    mesh, f = _case('hole')
    n = FacetNormal(mesh)
    expr = fem.traction(f['u'], f['p'], fem.Constant(MU))
    P = fem.BoundaryProfile(mesh, degree=10)     # a rule no other test uses
    calls = []
    upload = device.to_device
    monkeypatch.setattr(device, 'to_device',
                        lambda a: calls.append(1) or upload(a))
    first = P.evaluate(expr)
    assert len(calls) >= 4                      # the four lists, the rule
    del calls[:]
    again = P.evaluate(expr)
    assert torch.equal(first, again)
    out = torch.full_like(first, float('nan'))
    assert P.evaluate(expr, out=out) is out and torch.equal(out, first)
    a, b = P.cumulative(expr), P.cumulative(expr)
    assert torch.equal(a, b) and torch.equal(P.integrate(expr), P.integrate(expr))
    P.evaluate(dot(grad(f['th']), n))           # another program, the same rule
    assert calls == []
    with pytest.raises(ValueError, match='out'):
        P.evaluate(expr, out=out[:1])
    # nothing to do: nothing launched
    class Nowhere(fem.SubDomain):
        def inside(self, x, on_boundary):
            return on_boundary & (x[0] < -1.0)
    E = fem.BoundaryProfile(mesh, Nowhere())
    before = _hip.launch_count()
    assert tuple(E.evaluate(expr).shape) == (2, 0)
    assert tuple(E.cumulative(expr).shape) == (2, 0)
    assert tuple(E.total(expr).shape) == (2, 0)
    assert _hip.launch_count() == before


def test_c_abi_refusals_and_guarded_facets(hip):
    from flow_amd.fem import forms, ops
    mesh, f = _case('hole')
    P, _ = _pair('hole', 6)
    m, nf, npts = P.m, P.nfacets, P.npoints
    expr = fem.traction(f['u'], f['p'], MU)
    clean = _host(P.evaluate(expr))
    clean_int = _host(P.integrate(expr))
    prog = forms.compile_trees(expr.scalar_trees(), facet=True)
    fs, keep = ops._form_struct(prog, mesh, 6, True)
    ms = ctypes.byref(ops.mesh_struct(mesh))
    cell, local, dest, flip = P._lists()
    values = device.empty(2 * npts)
    integrals = device.empty(2 * nf)

    def call(form, n, cells, vals, ints=None):
        return hip.flow_form_facet_values(
            ms, ctypes.byref(form), n, _hip.i32(cells, nf), _hip.i32(local, nf),
            _hip.i32(dest, nf), _hip.i32(flip, nf),
            None if vals is None else _hip.f64(vals, 2 * npts),
            None if ints is None else _hip.f64(ints, 2 * nf), _hip.stream())

    before = _hip.launch_count()
    assert call(fs, nf, cell, None) == 2
    assert b'values' in hip.flow_last_error()
    assert call(fs, -1, cell, values) == 2
    assert b'facet count' in hip.flow_last_error()
    no_out = _hip.FormS()
    ctypes.memmove(ctypes.byref(no_out), ctypes.byref(fs), ctypes.sizeof(fs))
    for pc in range(no_out.nprog):
        if no_out.prog[4 * pc] == forms.OPS['out']:
            no_out.prog[4 * pc] = forms.OPS['mov']
            no_out.prog[4 * pc + 1] = 0
    assert call(no_out, nf, cell, values) == 2
    assert b'output' in hip.flow_last_error()
    assert call(fs, 0, cell, None) == 0
    assert _hip.launch_count() == before
    # a cell index == nc: NaN in that facet's samples and its integral, the
    # other entries as they were
    k = 17
    bad = _host(cell).copy()
    bad[k] = mesh.num_cells()
    d = int(_host(dest)[k])
    assert call(fs, nf, device.to_device(bad), values, integrals) == 0
    got = _host(values).reshape(2, npts)
    gint = _host(integrals).reshape(2, nf)
    hit = numpy.zeros(npts, dtype=bool)
    hit[d * m:(d + 1) * m] = True
    assert numpy.isnan(got[:, hit]).all() and numpy.isnan(gint[:, d]).all()
    assert numpy.array_equal(got[:, ~hit], clean[:, ~hit])
    assert numpy.array_equal(numpy.delete(gint, d, axis=1),
                             numpy.delete(clean_int, d, axis=1))
    del keep
