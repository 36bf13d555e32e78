# -*- coding: utf-8 -*-
'''
What tests/test_interior_facets_host.py and tests/test_interior_facets_gpu.py
share: the three fixture meshes (built once per process), fields given by
formulas, and the markers of a line of interior edges.
'''
import functools

import numpy

from flow_amd import fem
from flow_amd.fem import MeshFunction


@functools.lru_cache(maxsize=None)
def _fixtures():
    return (fem.UnitSquareMesh(3, 2, 'crossed'),
            fem.karman_channel_graded(lcar=2.0e-2),
            fem.karman_channel(60, 14, fitted=True))


def fixtures():
    '''Cells of both orientations and flip always 0 (24 cells, 31 interior
    facets); one orientation, both flip values, 7 distinct (local facet,
    neighbour's local facet, flip) triples (55, 66); the curved hole and
    several blocks (1648, 2390).'''
    return list(_fixtures())


def field(V, funcs):
    u = fem.Function(V)
    xy = V.layout.dof_coords
    u.set_array(numpy.concatenate([numpy.broadcast_to(
        f(xy[:, 0], xy[:, 1]), xy[:, 0].shape) for f in funcs]))
    return u


def x_half_markers(mesh):
    '''1 on the edges that lie on x == 0.5.'''
    m = MeshFunction('size_t', mesh, 1, 0)
    x = mesh.points[mesh.edges][:, :, 0]
    m.set_where((numpy.abs(x - 0.5) < 1e-12).all(axis=1), 1)
    return m
