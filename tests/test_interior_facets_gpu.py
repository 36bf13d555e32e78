# -*- coding: utf-8 -*-
'''
assemble(f*dS), interior_facet_integrals and cell_indicator on the HIP path
(csrc/form_kernels.hip: form_interior_facet_kernel, facet_cell_shares_kernel)
against the numpy evaluator of tests/interior_facet_reference.py, facts that
hold exactly, JumpIndicator, and a wrong list entry.
'''
import ctypes

import numpy
import pytest

from flow_amd import fem, _hip, device
from flow_amd.fem import (
    assemble, dx, ds, dS, Measure, FacetNormal, SpatialCoordinate,
    CellDiameter, CellVolume, Circumradius, FacetArea, jump, avg, dot, grad,
    inner, sqrt, conditional, gt, forms, ops,
    )

import interior_facet_reference as ifr
from interior_facet_cases import fixtures, field, x_half_markers

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def on():
    with fem.interior_facets(True):
        yield


def _fields(mesh):
    P1 = fem.FunctionSpace(mesh, 'CG', 1)
    P2 = fem.FunctionSpace(mesh, 'CG', 2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    p = field(P1, [lambda x, y: numpy.exp(x) * y + 2.0])
    th = field(P2, [lambda x, y: 0.5 + x * y + numpy.sin(9 * x)])
    w = field(W, [lambda x, y: numpy.sin(20 * x) * y + 1.0,
                  lambda x, y: numpy.cos(30 * y) * x])
    return p, th, w


def _integrands(mesh):
    p, th, w = _fields(mesh)
    n, X = FacetNormal(mesh), SpatialCoordinate(mesh)
    h, r, vol = CellDiameter(mesh), Circumradius(mesh), CellVolume(mesh)
    c = fem.Constant(1.7)
    six = inner(w('+'), w('-')) + jump(th) * avg(th)
    return [
        p * th + w[0],
        p('-') * th('+') - th('-'),
        jump(grad(p), n) * th,
        jump(grad(th), n)**2,
        dot(grad(w)('-'), n('+'))[0] * n('-')[1],
        jump(w, n) + dot(w('+'), n('+')),
        dot(jump(p, n), avg(grad(th))),
        avg(h) * jump(c * grad(th), n)**2,
        h('+') * r('-') + vol('+') / h('-') + r('+') * vol('-'),
        FacetArea(mesh) * X[0] * th('-') + X[1],
        sqrt(abs(jump(grad(p), n)) + 1.0) * abs(th('-')),
        # (the condition must not sit at rounding level: on the horizontal
        # edges of a structured mesh jump(grad(th), n) IS zero to rounding --
        # the P2 interpolant of a function of x alone does not depend on y
        # there -- and its sign would pick a branch at random)
        conditional(gt(th('-') * p('+'), 2.5), jump(grad(th), n), -p('-')),
        six,
        ]


def _scale(f, measure, mesh):
    return max(ifr.functional(abs(f) * measure),
               ifr.functional(fem.Constant(1.0) * measure(domain=mesh)))


def test_against_reference(hip):
    for mesh in fixtures():
        for f in _integrands(mesh):
            for measure in (dS, dS(degree=5)):
                got = assemble(f * measure)
                want = ifr.functional(f * measure)
                scale = _scale(f, measure, mesh)
                assert abs(got - want) <= 1e-12 * scale, (got, want, scale)
    # the NF = 6 and the EXT instances did run
    mesh = fixtures()[0]
    progs = [forms.compile_trees([(f * dS).integrand.comps], interior=True)
             for f in _integrands(mesh)]
    assert max(len(p.fields) for p in progs) == 6
    assert any(op == forms.OPS['select'] for p in progs
               for op, _, _, _ in p.code)


def test_marked_facets_and_signed_sums(hip):
    mesh = fixtures()[2]
    p, th, w = _fields(mesh)
    n = FacetNormal(mesh)
    m = fem.MeshFunction('size_t', mesh, 1, 0)
    mid = mesh.points[mesh.edges].mean(axis=1)
    m.set_where(mid[:, 0] < 0.2, 1)
    m.set_where(mid[:, 0] > 0.4, 2)
    dSm = Measure('dS', domain=mesh, subdomain_data=m)
    dsm = Measure('ds', domain=mesh, subdomain_data=m)
    f = jump(grad(th), n) * p + w[0]
    for k in (1, 2, 0):
        got, want = assemble(f * dSm(k)), ifr.functional(f * dSm(k))
        assert abs(got - want) <= 1e-12 * _scale(f, dSm(k), mesh)
    total = th * dx + f * dSm(1) - dot(w, n) * dsm(1) - avg(th) * dSm(2)
    scale = sum(abs(ifr.functional(part)) for _, part in total.terms())
    assert abs(assemble(total) - ifr.functional(total)) <= 1e-12 * scale
    assert assemble(f * dSm(7)) == 0.0


def test_exact_facts(hip):
    for mesh in fixtures():
        n = FacetNormal(mesh)
        P1 = fem.FunctionSpace(mesh, 'CG', 1)
        P2 = fem.FunctionSpace(mesh, 'CG', 2)
        u = field(P1, [lambda x, y: numpy.sin(6 * x) * y + x])
        v = field(P1, [lambda x, y: numpy.cos(4 * y) + x * y])
        u2 = field(P2, [lambda x, y: numpy.cos(7 * y) * x + 1.0])
        w = field(fem.VectorFunctionSpace(mesh, 'CG', 2),
                  [lambda x, y: x * y + 1.0, lambda x, y: numpy.sin(5 * x)])
        # jumps of continuous fields
        for f, mag in ((jump(u), abs(u)), (jump(u2)**2, u2**2),
                       (jump(w, n), sqrt(dot(w, w)))):
            assert abs(assemble(f * dS)) <= 1e-13 * assemble(mag * dS)
        # the flux jump of a global quadratic
        quad = field(P2, [lambda x, y: 1.0 + x - 2 * y + 3 * x * x - x * y
                          + 2 * y * y])
        got = assemble(abs(jump(grad(quad), n)) * dS)
        assert got <= 1e-12 * assemble(
            sqrt(dot(grad(quad)('+'), grad(quad)('+'))) * dS)
        # Green's identity
        scale = (assemble(abs(inner(grad(u), grad(v))) * dx)
                 + assemble(abs(jump(grad(u), n) * v) * dS)
                 + assemble(abs(dot(grad(u), n) * v) * ds))
        gap = assemble(inner(grad(u), grad(v)) * dx
                       - jump(grad(u), n) * v * dS - dot(grad(u), n) * v * ds)
        assert abs(gap) <= 1e-12 * scale, (gap, scale)
        # normals: n('+') + n('-') = 0 to rounding
        s = n('+') + n('-')
        length = assemble(fem.Constant(1.0) * dS(mesh))
        assert assemble(dot(s, s) * dS) <= 1e-26 * length
    # the flow rate through a marked line
    mesh = fem.UnitSquareMesh(4, 3)
    dSm = Measure('dS', domain=mesh, subdomain_data=x_half_markers(mesh))
    u = field(fem.VectorFunctionSpace(mesh, 'CG', 2),
              [lambda x, y: y * (1.0 - y), lambda x, y: 0.0 * x])
    assert abs(assemble(fem.Constant(1.0) * dSm(1)) - 1.0) <= 1e-12
    scale = assemble(abs(u[0]('+')) * dSm(1))
    for f in (u[0]('+'), u[0]('-'), u[0]):
        assert abs(assemble(f * dSm(1)) - 1.0 / 6.0) <= 1e-12 * scale


def test_determinism_and_empty_selection(hip):
    mesh = fixtures()[2]
    p, th, w = _fields(mesh)
    n = FacetNormal(mesh)
    f = avg(CellDiameter(mesh)) * jump(grad(th), n)**2 + p('-') * w[1]
    form = f * dS
    assert assemble(form) == assemble(form)
    a = device.to_host(fem.interior_facet_integrals(form)).numpy()
    b = device.to_host(fem.interior_facet_integrals(form)).numpy()
    assert a.shape == (len(mesh.interior_facets),) and numpy.array_equal(a, b)
    ids, want = ifr.facet_integrals(form)
    assert numpy.array_equal(ids, mesh.interior_facets)
    scale = _scale(f, dS, mesh)
    assert numpy.abs(a - want).max() <= 1e-12 * scale
    assert abs(a.sum() - assemble(form)) <= 1e-13 * scale
    e1 = device.to_host(fem.cell_indicator(form)).numpy()
    e2 = device.to_host(fem.cell_indicator(form)).numpy()
    assert numpy.array_equal(e1, e2)
    # an empty selection: exactly 0.0, nothing launched
    m = fem.MeshFunction('size_t', mesh, 1, 0)
    empty = f * Measure('dS', domain=mesh, subdomain_data=m)(5)
    before = _hip.launch_count()
    assert assemble(empty) == 0.0
    assert fem.interior_facet_integrals(empty).shape == (0,)
    assert _hip.launch_count() == before
    assert not device.to_host(fem.cell_indicator(empty)).numpy().any()


def test_cell_indicator(hip):
    for mesh in fixtures():
        p, th, w = _fields(mesh)
        n = FacetNormal(mesh)
        part = avg(CellDiameter(mesh)) * jump(grad(th), n)**2 * dS
        # the scale of the rounding: the jump is a difference of two O(1)
        # fluxes a and b that nearly cancel for this smooth field, and an
        # error eps in each moves (a - b)^2 by up to 2 eps (|a| + |b|)^2
        fluxes = abs(dot(grad(th)('+'), n('+'))) \
            + abs(dot(grad(th)('-'), n('-')))
        magnitude = avg(CellDiameter(mesh)) * fluxes**2 * dS
        for form, bound, share in (
                (part, magnitude, 0.5), (part, magnitude, 1.0),
                (part + th**2 * dx, magnitude + th**2 * dx, 0.5),
                (p * dx - part, abs(p) * dx + magnitude, 1.0),
                (-part + p * dx, magnitude + abs(p) * dx, 0.5),
                (-(p * dx) - part, abs(p) * dx + magnitude, 1.0)):
            got = device.to_host(fem.cell_indicator(form, share)).numpy()
            want = ifr.cell_shares(form, share)
            scale = ifr.cell_shares(bound, share).max()
            assert numpy.abs(got - want).max() <= 1e-12 * scale
        out = device.empty(mesh.num_cells())
        assert fem.cell_indicator(part, out=out) is out
        with pytest.raises(NotImplementedError, match='ds'):
            fem.cell_indicator(part + p * ds)
        # Kelly's indicator: the one formula JumpIndicator computes
        # (of fields whose flux jumps are of the size of the fluxes: max(eta2)
        # is then the scale of the rounding, not a square of a cancellation)
        for V in (p.function_space(), th.function_space()):
            u = field(V, [lambda x, y: numpy.sin(40 * x) * numpy.cos(25 * y)])
            kelly = FacetArea(mesh) / 24 * jump(grad(u), n)**2 * dS
            eta2 = fem.cell_indicator(kelly, share=1.0)
            ref = fem.JumpIndicator(V).apply(u)
            a = device.to_host(eta2).numpy()
            b = device.to_host(ref).numpy()
            assert numpy.abs(a - b).max() <= 1e-12 * b.max()
            # its output feeds fem.mark unchanged
            for strategy in ('dorfler', 'maximum'):
                mask = fem.mark(eta2, 0.4, strategy)
                assert mask.dtype == numpy.bool_ and mask.shape == a.shape
                if strategy == 'dorfler':
                    assert a[mask].sum() >= 0.4 * a.sum() * (1 - 1e-12)
                    assert a[mask].min() >= a[~mask].max() * (1 - 1e-12)
                # ... and selects the same cells
                assert numpy.array_equal(mask, fem.mark(ref, 0.4, strategy))


def test_bad_list_entries_give_nan(hip):
    '''A wrong-input check: every entry the kernel would use as an index is
    refused before it is used, so nothing is read outside an array.'''
    mesh = fixtures()[0]
    p, th, w = _fields(mesh)
    form = (jump(grad(th), FacetNormal(mesh)) * p + w[0]('-')) * dS
    L = mesh.interior_facet_lists()
    nc, nf = mesh.num_cells(), len(L['facets'])
    plus = L['cell_plus'].copy()
    local = L['local_plus'].copy()
    other = ((L['cell_minus'].astype(numpy.int64) << 3)
             | (L['local_minus'] << 1) | L['flip']).astype(numpy.int32)
    bad = {2: 'plus', 5: 'local', 7: 'other', 11: 'minus cell', 13: 'minus local',
           17: 'negative'}
    plus[2] = nc
    local[5] = 3
    other[7] = -1
    other[11] = (nc << 3) | (other[11] & 7)
    other[13] = other[13] | 6
    plus[17] = -4
    prog = forms.compile_trees([form.integrand.comps], interior=True)
    fs, keep = ops._form_struct(prog, mesh, form.degree(), True)
    out = device.empty(nf)
    dev = [device.to_device(a.astype(numpy.int32)) for a in (plus, local, other)]
    _hip.check(hip.flow_form_interior_facet_values(
        ctypes.byref(ops.mesh_struct(mesh)), ctypes.byref(fs), nf,
        _hip.i32(dev[0], nf), _hip.i32(dev[1], nf), _hip.i32(dev[2], nf),
        _hip.f64(out, nf), _hip.stream()))
    got = device.to_host(out).numpy()
    want = ifr.facet_integrals(form)[1]
    good = numpy.array([k not in bad for k in range(nf)])
    assert numpy.isnan(got[~good]).all()
    assert numpy.abs(got[good] - want[good]).max() <= 1e-12 * numpy.abs(want).max()
    # the entry points refuse a side bit, FacetArea's opcode and a slot read
    # on both sides where they do not belong
    res = ctypes.c_double(0.0)
    cells, loc, nb = ops.facet_lists(mesh)
    rc = hip.flow_form_facet_functional(
        ctypes.byref(ops.mesh_struct(mesh)), ctypes.byref(fs), nb,
        _hip.i32(cells, nb), _hip.i32(loc, nb),
        _hip.f64(ops.scratch(mesh, nb)), _hip.f64(ops.work(_hip.REDUCE_WORK)),
        ctypes.byref(res), _hip.stream())
    assert rc != 0 and b'interior facets only' in hip.flow_last_error()
    rc = hip.flow_form_functional(
        ctypes.byref(ops.mesh_struct(mesh)), ctypes.byref(fs),
        _hip.f64(ops.scratch(mesh, nc)), _hip.f64(ops.work(_hip.REDUCE_WORK)),
        ctypes.byref(res), _hip.stream())
    assert rc != 0
    del keep
