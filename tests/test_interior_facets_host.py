# -*- coding: utf-8 -*-
'''
Interior-facet integrals on the host (flow_amd/fem/forms.py: dS, jump, avg,
restrictions; Mesh.interior_facet_lists; ops.interior_facet_lists): the
switch and every refusal, the facet lists, the selection cache, the program
encoding, and the numpy evaluator of tests/interior_facet_reference.py
against facts that hold exactly.  No GPU.
'''
import json
import os

import numpy
import pytest

from flow_amd import fem, stabilization
from flow_amd.fem import (
    dx, ds, dS, Measure, MeshFunction, FacetNormal, SpatialCoordinate,
    CellDiameter, CellVolume, Circumradius, FacetArea, jump, avg, dot, grad,
    div, inner, sqrt, forms,
    )

import interior_facet_reference as ifr
from interior_facet_cases import fixtures, field, x_half_markers

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture
def on():
    with fem.interior_facets(True):
        yield


# -- 1. the switch and the refusals ---------------------------------------------
def test_switch_is_off_by_default_and_restores():
    assert fem.interior_facets.enabled is False
    with fem.interior_facets(True) as s:
        assert fem.interior_facets.enabled is True and s.previous is False
        with fem.interior_facets(False):
            assert fem.interior_facets.enabled is False
        assert fem.interior_facets.enabled is True
    assert fem.interior_facets.enabled is False


def test_everything_is_refused_while_off():
    mesh = fem.UnitSquareMesh(2, 2)
    u = fem.Function(fem.FunctionSpace(mesh, 'CG', 1))
    n = FacetNormal(mesh)
    attempts = [lambda: u * dS, lambda: dS(mesh), lambda: dS(1),
                lambda: Measure('dS'), lambda: Measure('dS', domain=mesh),
                lambda: jump(u), lambda: jump(u, n), lambda: avg(u),
                lambda: FacetArea(mesh), lambda: u('+'), lambda: u('-'),
                lambda: grad(u)('+'), lambda: n('-')]
    for attempt in attempts:
        with pytest.raises(NotImplementedError, match='dS') as e:
            attempt()
        assert 'interior_facets(True)' in str(e.value)


def test_measure_spellings(on):
    mesh = fem.UnitSquareMesh(2, 2)
    u = fem.Function(fem.FunctionSpace(mesh, 'CG', 2))
    m = x_half_markers(mesh)
    for measure in (dS, dS(mesh), dS(domain=mesh), Measure('dS'),
                    Measure('dS', domain=mesh, subdomain_data=m)(1),
                    Measure('interior_facet', domain=mesh)):
        form = u * measure
        assert form.integral_type == 'interior_facet' and form.rank == 0
    form = u * Measure('dS', domain=mesh, subdomain_data=m)(1)
    assert form.subdomain_id == 1 and form.subdomain_data is m
    # the degree: estimated as for ds, replaced as for ds
    assert (u**2 * dS).degree() == 4
    assert (u**2 * dS(degree=7)).degree() == 7
    assert (u**2 * dS(metadata={'quadrature_degree': 3})).degree() == 3
    assert (FacetArea(mesh) * u * dS).degree() == 2
    # dS(k) without markers: the ValueError of ds(k)
    with pytest.raises(ValueError, match='markers'):
        fem.ops.interior_facet_lists(mesh, None, 1)
    total = u * dx + u * ds - u('+') * dS
    assert [p.integral_type for _, p in total.terms()] == [
        'cell', 'exterior_facet', 'interior_facet']


def test_restriction_rules(on):
    mesh = fem.UnitSquareMesh(2, 2)
    P1 = fem.FunctionSpace(mesh, 'CG', 1)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    u, w = fem.Function(P1), fem.Function(W)
    n, X = FacetNormal(mesh), SpatialCoordinate(mesh)
    c = fem.Constant(2.0)
    # pushed down to the leaves: scalars, vectors, tensors
    assert u('+').comps == ('side', ('field', u, 0, 0), 0)
    assert u('-').comps == ('side', ('field', u, 0, 0), 1)
    assert grad(w)('-').shape == (2, 2)
    assert grad(w)('-').comps[1][0] == ('side', ('field', w, 1, 1), 1)
    assert grad(u('+')).comps == grad(u)('+').comps
    assert (c * X[0] * 3.0)('+').comps == (c * X[0] * 3.0).comps
    assert (u * c)('-').comps == ('mul', ('side', ('field', u, 0, 0), 1),
                                  ('const', c, 0))
    assert jump(u).comps == (u('+') - u('-')).comps
    assert jump(u, n).shape == (2,) and jump(w, n).shape == ()
    assert avg(w).shape == (2,) and avg(u).deg == 1
    assert jump(w, n).comps == (dot(w('+'), n('+'))
                                + dot(w('-'), n('-'))).comps
    # continuous operands may stand unrestricted: evaluated on '+'
    form = (u * X[0] * c * FacetArea(mesh) + w[1]) * dS
    assert forms.has_leaf(form.integrand.comps, 'side')
    assert (u * dS).integrand.comps == (u('+') * dS).integrand.comps
    # discontinuous ones must be restricted: ValueError naming the operand
    for f, word in ((grad(u)[0], 'gradient'), (n[0], 'FacetNormal'),
                    (div(w), 'gradient'), (CellVolume(mesh), 'CellVolume'),
                    (Circumradius(mesh), 'Circumradius'),
                    (CellDiameter(mesh) * u, 'CellDiameter')):
        with pytest.raises(ValueError, match=word):
            f * dS
    # a restriction under dx / ds, and of a restricted expression
    for measure in (dx, ds):
        with pytest.raises(ValueError, match='interior facets'):
            u('+') * measure
    with pytest.raises(ValueError, match='restricted'):
        u('+')('-')
    with pytest.raises(ValueError, match='restricted'):
        avg(u)('+')
    with pytest.raises(ValueError):
        forms.restricted(u, 'plus')
    with pytest.raises(ValueError, match='interior facets'):
        forms.Program([u('+').comps])
    with pytest.raises(ValueError, match='interior facets'):
        forms.point_program(u('-'))


def test_refused_with_the_switch_on(on):
    mesh = fem.UnitSquareMesh(2, 2)
    V = fem.FunctionSpace(mesh, 'CG', 1)
    u, v, du = fem.Function(V), fem.TestFunction(V), fem.TrialFunction(V)
    n = FacetNormal(mesh)
    for f in (u * v, du * v, jump(v) * u, avg(du) * avg(v), jump(grad(v), n)):
        with pytest.raises(NotImplementedError, match='dS'):
            f * dS
    e = fem.Expression('x[0]', degree=1)
    with pytest.raises(NotImplementedError, match='Expression'):
        e * u * dS
    tau = stabilization.supg(mesh, fem.Function(fem.VectorFunctionSpace(
        mesh, 'CG', 1)), 1.0e-2, 1)
    with pytest.raises(NotImplementedError, match='dS'):
        tau * u * dS
    for measure in (dx, ds):
        with pytest.raises(NotImplementedError, match='FacetArea'):
            FacetArea(mesh) * u * measure
    with pytest.raises(NotImplementedError, match='dS'):
        fem.derivative(u**2 * dS, u)
    with pytest.raises(NotImplementedError, match='dS'):
        fem.derivative(u**2 * dx + avg(u)**2 * dS, u)


def test_refused_on_strips(on, monkeypatch):
    '''dS on strips: each of the three device calls refuses before it
    compiles or launches anything.'''
    from flow_amd import parallel
    monkeypatch.setattr(parallel, 'active', lambda: True)
    mesh = fem.UnitSquareMesh(2, 2)
    u = fem.Function(fem.FunctionSpace(mesh, 'CG', 1))
    form = jump(grad(u), FacetNormal(mesh))**2 * dS
    for call in (fem.ops.assemble, fem.ops.interior_facet_integrals,
                 fem.ops.cell_indicator):
        with pytest.raises(NotImplementedError, match='on strips'):
            call(form)
    with pytest.raises(NotImplementedError, match='on strips'):
        fem.ops.assemble(u * dx + avg(u) * dS)
    with pytest.raises(NotImplementedError, match='on strips'):
        fem.ops.cell_indicator(u * dx + avg(u) * dS)


def test_refused_with_the_switch_off_too():
    '''What is refused with the switch on is refused with it off.'''
    mesh = fem.UnitSquareMesh(2, 2)
    V = fem.FunctionSpace(mesh, 'CG', 1)
    u, v = fem.Function(V), fem.TestFunction(V)
    with pytest.raises(NotImplementedError, match='dS'):
        u * v * dS
    with pytest.raises(NotImplementedError, match='dS'):
        fem.Expression('x[0]', degree=1) * dS


def test_function_call_stays_point_evaluation(on):
    mesh = fem.UnitSquareMesh(2, 2)
    u = fem.Function(fem.FunctionSpace(mesh, 'CG', 1))
    assert isinstance(u('+'), forms.FormExpr)
    # every other call is what it was: not a restriction
    for args in (('plus',), ('+', '-')):
        with pytest.raises(Exception) as e:
            u(*args)
        assert not isinstance(e.value, NotImplementedError)


# -- 2. the lists -------------------------------------------------------------
def test_fixtures_exercise_the_mapping():
    orientations, flips, triples = set(), set(), set()
    counts = []
    for mesh in fixtures():
        L = mesh.interior_facet_lists()
        counts.append((mesh.num_cells(), len(L['facets'])))
        p = mesh.points[mesh.cell_vertices]
        d1, d2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        orientations |= set(numpy.sign(
            d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]).tolist())
        flips |= set(L['flip'].tolist())
        triples |= set(zip(L['local_plus'].tolist(),
                           L['local_minus'].tolist(), L['flip'].tolist()))
    assert counts == [(24, 31), (55, 66), (1648, 2390)]
    assert orientations == {-1.0, 1.0}
    assert flips == {0, 1}
    assert len(triples) >= 7


def test_list_properties():
    for mesh in fixtures():
        L = mesh.interior_facet_lists()
        facets = L['facets']
        assert numpy.array_equal(facets, mesh.interior_facets)
        assert (numpy.diff(facets) > 0).all()
        assert not set(facets.tolist()) & set(mesh.bfacets.tolist())
        assert len(facets) + len(mesh.bfacets) == mesh.num_edges()
        ce = mesh.cell_edges
        assert numpy.array_equal(ce[L['cell_plus'], L['local_plus']], facets)
        assert numpy.array_equal(ce[L['cell_minus'], L['local_minus']], facets)
        assert (L['cell_plus'] < L['cell_minus']).all()
        # the flip bit: the facet's first vertex in '-' against '+'
        first = numpy.array([1, 0, 0])
        second = numpy.array([2, 2, 1])
        cv = mesh.cell_vertices
        p0 = cv[L['cell_plus'], first[L['local_plus']]]
        p1 = cv[L['cell_plus'], second[L['local_plus']]]
        m0 = cv[L['cell_minus'], first[L['local_minus']]]
        m1 = cv[L['cell_minus'], second[L['local_minus']]]
        f = L['flip'].astype(bool)
        assert numpy.array_equal(numpy.where(f, m1, m0), p0)
        assert numpy.array_equal(numpy.where(f, m0, m1), p1)
        # against the evaluator's own search, and adapt.facet_table's packing
        ids, cells = ifr.two_cell_edges(mesh)
        assert numpy.array_equal(ids, facets)
        assert numpy.array_equal(cells[:, 0], L['cell_plus'])
        assert numpy.array_equal(cells[:, 1], L['cell_minus'])
        table = fem.adapt.facet_table(mesh)
        nc = mesh.num_cells()
        packed = (L['cell_minus'].astype(numpy.int64) << 3) \
            | (L['local_minus'] << 1) | L['flip']
        assert numpy.array_equal(
            table[L['local_plus'].astype(numpy.int64) * nc + L['cell_plus']],
            packed)
        # total length: (sum of the cell perimeters - boundary length) / 2
        ev = mesh.edges
        length = numpy.hypot(*(mesh.points[ev[:, 1]] - mesh.points[ev[:, 0]]).T)
        want = 0.5 * (mesh._edge_lengths().sum() - length[mesh.bfacets].sum())
        assert abs(length[facets].sum() - want) <= 1e-14 * want


# -- 3. the selection cache ---------------------------------------------------
def test_selection_cache(monkeypatch):
    from flow_amd import device
    monkeypatch.setattr(device, 'to_device', lambda a: numpy.array(a))
    mesh = fem.UnitSquareMesh(4, 3)
    every = fem.ops.interior_facet_lists(mesh)
    assert every is fem.ops.interior_facet_lists(mesh, None, 'everywhere')
    assert every.count == len(mesh.interior_facets)
    assert numpy.array_equal(numpy.nonzero(every.positions >= 0)[0],
                             mesh.interior_facets)
    m = x_half_markers(mesh)
    one = fem.ops.interior_facet_lists(mesh, m, 1)
    assert one is fem.ops.interior_facet_lists(mesh, m, 1)
    assert one.count == 3
    # the cell gather's map: the selected facets of every cell, else -1
    nc = mesh.num_cells()
    cp = numpy.asarray(one.cell_positions).reshape(3, nc)
    assert numpy.array_equal(cp, one.positions[mesh.cell_edges].T)
    assert (cp >= 0).sum() == 2 * one.count
    # an unused id selects nothing and holds no device array
    none = fem.ops.interior_facet_lists(mesh, m, 7)
    assert none.count == 0 and none.plus is None and none.other is None
    assert (none.positions == -1).all()
    # boundary facets carry markers too, and are never selected
    m.set_all(1)
    all_marked = fem.ops.interior_facet_lists(mesh, m, 1)
    assert all_marked is not one and all_marked.count == every.count
    # re-marking bumps the selection
    m.set_all(0)
    m[int(mesh.interior_facets[5])] = 1
    again = fem.ops.interior_facet_lists(mesh, m, 1)
    assert again.count == 1
    assert again.positions[mesh.interior_facets[5]] == 0
    with pytest.raises(ValueError, match='another mesh'):
        fem.ops.interior_facet_lists(fem.UnitSquareMesh(2, 2), m, 1)


# -- 4. the program encoding --------------------------------------------------
def test_programs_without_restrictions_are_byte_for_byte_the_parents():
    import form_program_digests
    with open(os.path.join(HERE, 'golden', 'form_program_digests.json')) as f:
        want = json.load(f)
    assert len(want) > 80
    assert form_program_digests.digests() == want
    with fem.interior_facets(True):
        assert form_program_digests.digests() == want


def test_side_bits_and_slots(on):
    mesh = fem.UnitSquareMesh(2, 2)
    P2 = fem.FunctionSpace(mesh, 'CG', 2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 1)
    u, w = fem.Function(P2), fem.Function(W)
    n, h = FacetNormal(mesh), CellDiameter(mesh)
    OPS = forms.OPS
    assert OPS['facet_len'] == 29 and forms.SIDE_BIT == {
        'field': 4, 'normal': 2, 'cell': 4}
    form = (jump(u) + grad(u)('-')[1] * n('-')[1] * h('-') + n('+')[0]
            * h('+') * FacetArea(mesh) + u) * dS
    prog = forms.compile_trees([form.integrand.comps], interior=True)
    # u('+') and u('-') take two slots; the unrestricted u shares '+'
    assert prog.fields == [(u, 0), (u, 0)]
    assert sorted(prog.field_sides) == [0, 1]
    leaves = set((op, a, b) for op, _, a, b in prog.code
                 if op in (OPS['field'], OPS['normal'], OPS['cell'],
                           OPS['facet_len']))
    plus, minus = prog.field_sides.index(0), prog.field_sides.index(1)
    assert leaves == {
        (OPS['field'], plus, 0), (OPS['field'], minus, 4),
        (OPS['field'], minus, 2 | 4), (OPS['normal'], 1 | 2, 0),
        (OPS['normal'], 0, 0), (OPS['cell'], 2 | 4, 0), (OPS['cell'], 2, 0),
        (OPS['facet_len'], 0, 0)}
    # without a restriction the interior program is the exterior one
    plain = fem.sin(u) * u * dS
    a = forms.compile_trees([plain.integrand.comps], interior=True)
    b = forms.compile_trees([(fem.sin(u) * u).comps], facet=True)
    assert a.code == b.code and a.field_sides == [0] and b.field_sides is None
    # six slots fit, the seventh is a ProgramLimit
    six = (inner(w('+'), w('-')) + jump(u) * avg(u)) * dS
    p6 = forms.compile_trees([six.integrand.comps], interior=True)
    assert len(p6.fields) == 6 == forms.MAX_FIELDS
    assert sorted(p6.field_sides) == [0, 0, 0, 1, 1, 1]
    p = fem.Function(fem.FunctionSpace(mesh, 'CG', 1))
    seven = (inner(w('+'), w('-')) + jump(u) * avg(u) + p('-')) * dS
    with pytest.raises(forms.ProgramLimit, match='field components'):
        forms.compile_trees([seven.integrand.comps], interior=True)
    assert issubclass(forms.ProgramLimit, ValueError)


# -- 5. the reference against exact facts -------------------------------------
def _scale(*forms_):
    return sum(ifr.functional(f) for f in forms_)


def test_reference_jumps_of_continuous_fields_vanish(on):
    for mesh in fixtures()[:2]:
        n = FacetNormal(mesh)
        u1 = field(fem.FunctionSpace(mesh, 'CG', 1),
                   [lambda x, y: numpy.sin(9 * x) + y])
        u2 = field(fem.FunctionSpace(mesh, 'CG', 2),
                   [lambda x, y: numpy.cos(7 * y) * x + 1.0])
        w = field(fem.VectorFunctionSpace(mesh, 'CG', 2),
                  [lambda x, y: x * y + 1.0, lambda x, y: numpy.sin(5 * x)])
        for f, mag in ((jump(u1), abs(u1)), (jump(u2)**2, u2**2),
                       (jump(w, n), sqrt(dot(w, w))),
                       (jump(w)[0] + jump(w)[1], sqrt(dot(w, w)))):
            got = ifr.functional(f * dS)
            assert abs(got) <= 1e-13 * ifr.functional(mag * dS), got


def test_reference_flux_jump_of_a_global_quadratic_vanishes(on):
    for mesh in fixtures()[:2]:
        n = FacetNormal(mesh)
        u = field(fem.FunctionSpace(mesh, 'CG', 2),
                  [lambda x, y: 1.0 + x - 2 * y + 3 * x * x - x * y + 2 * y * y])
        got = ifr.functional(abs(jump(grad(u), n)) * dS)
        scale = ifr.functional(sqrt(dot(grad(u)('+'), grad(u)('+'))) * dS)
        assert abs(got) <= 1e-12 * scale, (got, scale)


def test_reference_greens_identity(on):
    for mesh in fixtures()[:2]:
        n = FacetNormal(mesh)
        P1 = fem.FunctionSpace(mesh, 'CG', 1)
        u = field(P1, [lambda x, y: numpy.sin(6 * x) * y + x])
        v = field(P1, [lambda x, y: numpy.cos(4 * y) + x * y])
        vol = inner(grad(u), grad(v)) * dx
        inn = jump(grad(u), n) * v * dS
        ext = dot(grad(u), n) * v * ds
        scale = _scale(abs(inner(grad(u), grad(v))) * dx,
                       abs(jump(grad(u), n) * v) * dS,
                       abs(dot(grad(u), n) * v) * ds)
        gap = ifr.functional(vol) - ifr.functional(inn) - ifr.functional(ext)
        assert abs(gap) <= 1e-12 * scale, (gap, scale)
        assert abs(ifr.functional(vol - inn - ext)) <= 1e-12 * scale


def test_reference_flow_rate_through_a_marked_line(on):
    mesh = fem.UnitSquareMesh(4, 3)
    m = x_half_markers(mesh)
    dSm = Measure('dS', domain=mesh, subdomain_data=m)
    u = field(fem.VectorFunctionSpace(mesh, 'CG', 2),
              [lambda x, y: y * (1.0 - y), lambda x, y: 0.0 * x])
    one = ifr.functional(fem.Constant(1.0) * dSm(1))
    assert abs(one - 1.0) <= 1e-12
    scale = ifr.functional(abs(u[0]('+')) * dSm(1))
    for f in (u[0]('+'), u[0]('-'), u[0], avg(u)[0]):
        assert abs(ifr.functional(f * dSm(1)) - 1.0 / 6.0) <= 1e-12 * scale
    assert ifr.functional(u[0] * dSm(2)) == 0.0
    # per cell: every cell on the line gets half of its facet
    shares = ifr.cell_shares(u[0] * dSm(1), 0.5)
    assert abs(shares.sum() - 1.0 / 6.0) <= 1e-12 * scale
    assert (shares != 0.0).sum() == 6
