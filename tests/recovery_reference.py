# -*- coding: utf-8 -*-
'''
Host restatement of flow_amd/fem/recovery.py in numpy, independent of the
kernels and of the space's contribution map (vptr / vsrc): the patches come
from `cell_dofs`, the geometry from `mesh.cell_vertices` and `mesh.points`,
the P1 / P2 basis and its gradients are written out below in the reference
coordinates (xi, eta), and the cell integrals use Dunavant's 6-point rule
(exact to degree 4), not reference.triangle_rule.

    G_k(n) = sum_c |T_c| grad u_k|_c(x_n) / sum_c |T_c|   over the cells with
             node n, each patch summed in ASCENDING CELL order
    eta2[c] = sum_k int_T |G_k - grad u_k|^2 dx
'''
import numpy

# the reference position of local node i: the vertices, then the mid points of
# the edges opposite vertex 0, 1, 2
NODES = numpy.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0],
                     [0.5, 0.5], [0.0, 0.5], [0.5, 0.0]])

# Dunavant, degree 4: barycentric (a, a, 1 - 2a) permuted, weights sum to 1
_A1, _W1 = 0.445948490915965, 0.223381589678011
_A2, _W2 = 0.091576213509771, 0.109951743655322
RULE_POINTS = numpy.array([
    [_A1, _A1], [_A1, 1 - 2 * _A1], [1 - 2 * _A1, _A1],
    [_A2, _A2], [_A2, 1 - 2 * _A2], [1 - 2 * _A2, _A2]])
RULE_WEIGHTS = numpy.array([_W1, _W1, _W1, _W2, _W2, _W2])


def basis(degree, pts):
    '''Values (npts, nloc) of the basis at reference points (npts, 2).'''
    xi, eta = pts[:, 0], pts[:, 1]
    lam = 1.0 - xi - eta
    if degree == 1:
        return numpy.stack([lam, xi, eta], axis=1)
    return numpy.stack([lam * (2 * lam - 1), xi * (2 * xi - 1),
                        eta * (2 * eta - 1), 4 * xi * eta, 4 * eta * lam,
                        4 * xi * lam], axis=1)


def basis_grad(degree, pts):
    '''d/d(xi, eta) of the basis: (npts, nloc, 2).'''
    xi, eta = pts[:, 0], pts[:, 1]
    one, zero = numpy.ones_like(xi), numpy.zeros_like(xi)
    if degree == 1:
        return numpy.stack([numpy.stack([-one, -one], axis=1),
                            numpy.stack([one, zero], axis=1),
                            numpy.stack([zero, one], axis=1)], axis=1)
    lam = 1.0 - xi - eta
    d0 = 1.0 - 4.0 * lam
    return numpy.stack([
        numpy.stack([d0, d0], axis=1),
        numpy.stack([4 * xi - 1, zero], axis=1),
        numpy.stack([zero, 4 * eta - 1], axis=1),
        numpy.stack([4 * eta, 4 * xi], axis=1),
        numpy.stack([-4 * eta, 4 * (lam - eta)], axis=1),
        numpy.stack([4 * (lam - xi), -4 * xi], axis=1)], axis=1)


def _geometry(mesh):
    '''(J^-T (nc, 2, 2) mapping reference to physical gradients, areas).'''
    P = mesh.points[mesh.cell_vertices]                          # (nc, 3, 2)
    J = numpy.stack([P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]], axis=2)
    det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
    return numpy.linalg.inv(J).transpose(0, 2, 1), 0.5 * numpy.abs(det)


def cell_gradients(V, U, pts):
    '''grad u_k of every cell at its reference points pts: (dim, nc, npts, 2);
    U: (dim, N).'''
    JinvT, _ = _geometry(V.mesh())
    Uc = U[:, V.layout.cell_dofs]                                # (dim, nc, nloc)
    gref = numpy.einsum('kcj,qjr->kcqr', Uc, basis_grad(V.degree, pts))
    return numpy.einsum('cdr,kcqr->kcqd', JinvT, gref)


def patches(V):
    '''For every node the sorted list of its (local node, cell) pairs.'''
    out = [[] for _ in range(V.N)]
    for c, dofs in enumerate(V.layout.cell_dofs):
        for i, n in enumerate(dofs):
            out[n].append((i, c))
    return out


def gradient(u):
    '''The recovered gradient of the Function u: (dim, 2, N).'''
    V = u.function_space()
    U = u.array().reshape(V.dim, V.N)
    nloc = V.layout.cell_dofs.shape[1]
    g = cell_gradients(V, U, NODES[:nloc])                       # (dim, nc, nloc, 2)
    _, area = _geometry(V.mesh())
    nodes = V.layout.cell_dofs.ravel()                           # cell-major
    wsum = numpy.zeros(V.N)
    numpy.add.at(wsum, nodes, numpy.repeat(area, nloc))
    G = numpy.zeros((V.dim, 2, V.N))
    for k in range(V.dim):
        for d in range(2):
            # add.at adds in the order of `nodes`: ascending cells
            numpy.add.at(G[k, d], nodes, (area[:, None] * g[k, :, :, d]).ravel())
    return G / wsum


def indicator(u, G=None):
    '''eta2 (nc,) of the Function u, with G (dim, 2, N) = gradient(u).'''
    V = u.function_space()
    U = u.array().reshape(V.dim, V.N)
    G = gradient(u) if G is None else G
    _, area = _geometry(V.mesh())
    gu = cell_gradients(V, U, RULE_POINTS)                       # (dim, nc, nq, 2)
    phi = basis(V.degree, RULE_POINTS)                           # (nq, nloc)
    Gc = G[:, :, V.layout.cell_dofs]                             # (dim, 2, nc, nloc)
    Gq = numpy.einsum('kdcj,qj->kcqd', Gc, phi)
    return area * numpy.einsum('kcqd,q->c', (Gq - gu)**2, RULE_WEIGHTS)


def field(V, funcs):
    '''The Function on V with the nodal values of funcs (one per component).'''
    from flow_amd import fem
    u = fem.Function(V)
    xy = V.layout.dof_coords
    u.set_array(numpy.concatenate(
        [numpy.broadcast_to(f(xy[:, 0], xy[:, 1]), (V.N,)) for f in funcs]))
    return u


# -- H1-seminorm errors on the host (the superconvergence check) -----------------
def gradient_errors(u, exact_grad):
    '''(|G - grad u_exact|_L2, |grad u_h - grad u_exact|_L2) of a scalar
    Function u; exact_grad(x, y) -> (gx, gy).  G interpolated in P_deg,
    integrals by the rule above on every cell.'''
    V = u.function_space()
    mesh = V.mesh()
    U = u.array().reshape(1, V.N)
    G = gradient(u)
    _, area = _geometry(mesh)
    P = mesh.points[mesh.cell_vertices]
    lam = numpy.stack([1 - RULE_POINTS.sum(axis=1), RULE_POINTS[:, 0],
                       RULE_POINTS[:, 1]], axis=1)               # (nq, 3)
    X = numpy.einsum('qv,cvd->cqd', lam, P)
    ge = numpy.stack(exact_grad(X[:, :, 0], X[:, :, 1]), axis=2)  # (nc, nq, 2)
    gu = cell_gradients(V, U, RULE_POINTS)[0]
    Gq = numpy.einsum('dcj,qj->cqd', G[0][:, V.layout.cell_dofs],
                      basis(V.degree, RULE_POINTS))
    rec = numpy.sqrt((area * numpy.einsum('cqd,q->c', (Gq - ge)**2,
                                          RULE_WEIGHTS)).sum())
    raw = numpy.sqrt((area * numpy.einsum('cqd,q->c', (gu - ge)**2,
                                          RULE_WEIGHTS)).sum())
    return rec, raw


# -- the meshes and fields the host and the GPU tests share ---------------------
MESHES = ('square 2', 'hole', 'fitted hole', 'hole refined', 'square 24')
_HELD = {}


def mesh(name):
    '''square 2: one interior node, every other patch one-sided; hole:
    rectangle_with_hole's staircase (re-entrant corners, patches of one to
    eight cells); fitted hole: its body-fitted variant -- stretched cells of
    mixed valence, a polygon on the circle as boundary; hole refined: that
    mesh after one refine() of about a third of its cells (the valences
    bisection produces, new boundary nodes moved onto the circle); square
    24: with P2 2401 nodes and 1152 cells, several blocks and a ragged tail
    for the node kernel and for the cell kernel.'''
    from flow_amd import fem
    if name not in _HELD:
        if name == 'square 2':
            m = fem.UnitSquareMesh(2, 2)
        elif name == 'square 24':
            m = fem.UnitSquareMesh(24, 24)
        elif name == 'hole':
            m = fem.rectangle_with_hole(0.0, 1.0, 0.0, 0.5, (0.4, 0.25), 0.12,
                                        12, 6)
        elif name == 'fitted hole':
            m = fem.mesh.rectangle_with_fitted_hole(
                0.0, 1.0, 0.0, 0.5, (0.4, 0.25), 0.1, 16, 8)
        else:
            assert name == 'hole refined'
            coarse = mesh('fitted hole')
            rng = numpy.random.RandomState(3)
            m = fem.refine(coarse, rng.uniform(size=coarse.num_cells()) < 1.0 / 3.0)
        _HELD[name] = m
    return _HELD[name]


# Smooth, non-polynomial, and oscillatory enough that G - grad u_h stays above
# 1e-2 |G| in the cell with the largest eta2 on every mesh above, P2 included:
# eta2 is a sum of squares of that DIFFERENCE, so its relative rounding is
# about 1e-15 |G| / |G - grad u_h| whoever computes it (with sin(3x + 1)
# exp(y) on 'square 24', P2, two numpy evaluations of the same formula with
# different exact rules already differ by 1.6e-11 of max eta2).
def smooth0(x, y):
    return numpy.sin(29 * x + 1) * numpy.exp(y)


def smooth1(x, y):
    return numpy.cos(27 * y - 4 * x) * (1 + x * x)


# global polynomials of degree 1 and 2 with their gradients
def linear(x, y):
    return 3 + x - 2 * y


def quadratic(x, y):
    return 1 + 2 * x - 3 * y + 0.5 * x * x + x * y - 2 * y * y


def quadratic_grad(x, y):
    return 2 + x + y, -3 + x - 4 * y


def quadratic1(x, y):
    return x * x - y * x + y


def quadratic1_grad(x, y):
    return 2 * x - y, 1 - x


# (degree, funcs, their gradients, max |grad u| on the unit square)
EXACT = {
    (1, 1): ([linear], [lambda x, y: (1 + 0 * x, -2 + 0 * x)], 2.3),
    (2, 1): ([quadratic], [quadratic_grad], 7.0),
    (1, 2): ([linear, lambda x, y: 0.5 * y - x],
             [lambda x, y: (1 + 0 * x, -2 + 0 * x),
              lambda x, y: (-1 + 0 * x, 0.5 + 0 * x)], 2.3),
    (2, 2): ([quadratic, quadratic1], [quadratic_grad, quadratic1_grad], 7.0),
    }


def bubble(x, y):
    return numpy.sin(numpy.pi * x) * numpy.sin(numpy.pi * y)


def bubble_grad(x, y):
    return (numpy.pi * numpy.cos(numpy.pi * x) * numpy.sin(numpy.pi * y),
            numpy.pi * numpy.sin(numpy.pi * x) * numpy.cos(numpy.pi * y))
