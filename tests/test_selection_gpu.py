# -*- coding: utf-8 -*-
'''
Selections on the GPU (flow_amd/fem/selection.py behind ops.assemble and a
held ops.NewtonAssembler): ds(1) and dx(1) parts of rank 1 and 2 on a P1 and a
P2 scalar space, a P2 vector space and the Taylor-Hood space, assembled,
assembled again after one facet and one cell were re-marked, and once more.
Every result is compared bit for bit with an assembly from a freshly built
mesh, markers and spaces that carry that marking from the start: this code
decides indices and order only, so there is no tolerance.  UnitSquareMesh(4,
3): interior cells, several boundary facets per side, a marked subset that is
neither empty nor everything.
'''
import numpy
import pytest
import torch

from flow_amd import fem
from flow_amd.fem import (
    TestFunction, TrialFunction, TestFunctions, TrialFunctions, assemble, dx,
    Measure, MeshFunction, SpatialCoordinate, FacetNormal, dot, inner, grad,
    div, derivative, ops,
    )

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _switches_on():
    with fem.mixed_arguments(True), fem.vector_arguments(True), \
            fem.facet_arguments(True), fem.cell_subdomains(True):
        yield


class Setup(object):
    '''A fresh mesh with facet and cell markers: id 1 on every second
    boundary facet and every third cell; `final`: also on the facet and the
    cell that remark() adds.'''

    def __init__(self, final=False):
        self.mesh = mesh = fem.UnitSquareMesh(4, 3)
        self.facets = MeshFunction('size_t', mesh, 1, 0)
        self.cells = MeshFunction('size_t', mesh, 2, 0)
        for f in mesh.bfacets[::2]:
            self.facets[int(f)] = 1
        for c in range(0, mesh.num_cells(), 3):
            self.cells[c] = 1
        self.ds = Measure('ds', domain=mesh, subdomain_data=self.facets)
        self.dx = Measure('dx', domain=mesh, subdomain_data=self.cells)
        if final:
            self.remark()

    def remark(self):
        self.facets[int(self.mesh.bfacets[1])] = 1
        self.cells[1] = 1


def _scalar_forms(degree):
    def forms(s):
        V = fem.FunctionSpace(s.mesh, 'CG', degree)
        u, v = TrialFunction(V), TestFunction(V)
        x = SpatialCoordinate(s.mesh)
        c = 1.0 + x[0] * x[1]
        return [c * v * s.ds(1), c * v * s.dx(1), c * u * v * s.ds(1),
                c * inner(grad(u), grad(v)) * s.dx(1) + u * v * s.dx(1)]
    return forms


def _vector_forms(s):
    W = fem.VectorFunctionSpace(s.mesh, 'CG', 2)
    u, v = TrialFunction(W), TestFunction(W)
    x = SpatialCoordinate(s.mesh)
    c = 1.0 + x[0] * x[1]
    return [dot(c * x, v) * s.ds(1), dot(c * x, v) * s.dx(1),
            c * dot(u, v) * s.ds(1), c * inner(grad(u), grad(v)) * s.dx(1)]


def _taylor_hood_forms(s):
    WP = fem.FunctionSpace(
        s.mesh, fem.VectorElement('Lagrange', 'triangle', 2)
        * fem.FiniteElement('Lagrange', 'triangle', 1))
    (u, p), (v, q) = TrialFunctions(WP), TestFunctions(WP)
    x = SpatialCoordinate(s.mesh)
    n = FacetNormal(s.mesh)
    c = 1.0 + x[0] * x[1]
    # (every block of the mixed table under both measures: the velocity
    # corner, the pressure corner and the coupling planes' list launches)
    return [dot(c * x, v) * s.ds(1) + c * q * s.ds(1),
            dot(c * x, v) * s.dx(1) + c * q * s.dx(1),
            c * dot(u, v) * s.ds(1) + p * dot(v, n) * s.ds(1)
            + q * dot(u, n) * s.ds(1) + c * p * q * s.ds(1),
            3.0 * dot(u, v) * s.dx(1) - p * div(v) * s.dx(1)
            - q * div(u) * s.dx(1) + c * q * u[1] * s.dx(1)
            + c * p * q * s.dx(1)]


SPACES = {'P1': _scalar_forms(1), 'P2': _scalar_forms(2),
          'P2 vector': _vector_forms, 'Taylor-Hood': _taylor_hood_forms}
NAMES = ['rank 1 ds(1)', 'rank 1 dx(1)', 'rank 2 ds(1)', 'rank 2 dx(1)']


def _values(result):
    '''Copies of the device values of a Vector, a Matrix or a MixedMatrix (or
    of a held assembler's plain tensor).'''
    if isinstance(result, torch.Tensor):
        return [result.clone()]
    if hasattr(result, 'blocks'):
        blocks = result.blocks()
        assert blocks
        return [B.vals.clone() for _, B in blocks]
    return [(result.vals if hasattr(result, 'vals') else result.data).clone()]


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('space', sorted(SPACES))
def test_assemble_follows_the_markers(hip, space):
    build = SPACES[space]
    held = Setup()
    forms = build(held)
    first = [_values(assemble(f)) for f in forms]
    held.remark()
    second = [_values(assemble(f)) for f in forms]
    third = [_values(assemble(f)) for f in forms]
    initial = [_values(assemble(f)) for f in build(Setup())]
    final = [_values(assemble(f)) for f in build(Setup(final=True))]
    for k, name in enumerate(NAMES):
        what = '%s, %s' % (space, name)
        assert _equal(first[k], initial[k]), what
        assert _equal(second[k], final[k]), what
        assert _equal(third[k], second[k]), what
        # (... and the re-marking is seen at all)
        assert not _equal(second[k], first[k]), what
        assert all(bool(torch.isfinite(v).all()) and bool((v != 0.0).any())
                   for v in second[k]), what


def _newton(s):
    '''A held assembler of a residual with a ds(1) and a dx(1) part.'''
    V = fem.FunctionSpace(s.mesh, 'CG', 2)
    u = fem.Function(V)
    xy = V.layout.dof_coords
    u.set_array(1.5 + 0.5 * numpy.sin(3.0 * xy[:, 0]) * numpy.cos(2.0 * xy[:, 1]))
    v = TestFunction(V)
    F = 0.8 * dot(grad(u), grad(v)) * dx - v * dx + 0.3 * u**4 * v * s.ds(1) \
        + u * u * v * s.dx(1)
    asm = ops.NewtonAssembler(derivative(F, u), F, V)
    assert asm.route == 'by_parts'
    return asm, u


def _newton_values(asm):
    A, b = asm.assemble()
    return _values(A) + _values(b)


def test_held_assembler_follows_the_markers(hip):
    '''_FacetTarget: the held buffers are zeroed again where the map is
    another one, so the entries of the facet and the cell that were added
    come on top of zeros, and nothing of the first marking is left.'''
    held = Setup()
    asm, u = _newton(held)
    first = _newton_values(asm)
    held.remark()
    second = _newton_values(asm)
    third = _newton_values(asm)
    fresh, ufresh = _newton(Setup())
    initial = _newton_values(fresh)
    fresh, ufresh = _newton(Setup(final=True))
    final = _newton_values(fresh)
    assert _equal(first, initial)
    assert _equal(second, final)
    assert _equal(third, second)
    assert not torch.equal(second[0], first[0])
    assert not torch.equal(second[1], first[1])
    # ... and back: un-marking leaves nothing behind either
    held.facets[int(held.mesh.bfacets[1])] = 0
    held.cells[1] = 0
    assert _equal(_newton_values(asm), initial)
    del u, ufresh
