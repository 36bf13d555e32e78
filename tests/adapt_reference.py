# -*- coding: utf-8 -*-
'''
Host evaluator of the jump indicator of flow_amd/fem/adapt.py: numpy,
independent of the kernel and of its facet table.  It walks `mesh.edges`,
finds the two cells of every interior edge through an edge -> cells map of
its own (built from `cell_vertices`, not from `mesh.cell_neighbors`), puts
Gauss-Legendre points on the edge in physical coordinates, inverts each
cell's affine map there and evaluates the gradients with
`reference.tabulate_grad`, as tests/facet_reference.py does, and adds
|E| / 24 * int_E sum_k [grad u_k . n]^2 ds to both cells.

Also the pieces the adaptive-loop tests share: the manufactured Poisson
problem, L2 errors against its exact solution and the uniform baseline.
'''
import numpy

from flow_amd.fem import reference


def edge_cells(mesh):
    '''(interior edge ids (m,), their two cells (m, 2)): each cell's three
    vertex pairs looked up among the sorted pairs of mesh.edges.'''
    cv = mesh.cell_vertices.astype(numpy.int64)
    nv = mesh.num_vertices()
    ekey = mesh.edges[:, 0].astype(numpy.int64) * nv + mesh.edges[:, 1]
    assert (numpy.diff(ekey) > 0).all()
    found, owner = [], []
    for a, b in ((0, 1), (1, 2), (2, 0)):
        lo = numpy.minimum(cv[:, a], cv[:, b])
        hi = numpy.maximum(cv[:, a], cv[:, b])
        e = numpy.searchsorted(ekey, lo * nv + hi)
        assert numpy.array_equal(ekey[e], lo * nv + hi)
        found.append(e)
        owner.append(numpy.arange(len(cv)))
    found, owner = numpy.concatenate(found), numpy.concatenate(owner)
    order = numpy.argsort(found, kind='stable')
    found, owner = found[order], owner[order]
    count = numpy.bincount(found, minlength=len(ekey))
    assert count.min() >= 1 and count.max() <= 2
    start = numpy.cumsum(count) - count
    inner = numpy.nonzero(count == 2)[0]
    pairs = numpy.stack([owner[start[inner]], owner[start[inner] + 1]], axis=1)
    return inner, pairs.reshape(-1, 2)


def _gradients(V, U, cells, X):
    '''grad u_k at the points X (m, nq, 2) of the cells (m,): (dim, m, nq, 2).'''
    mesh = V.mesh()
    P = mesh.points[mesh.cell_vertices[cells]]                  # (m, 3, 2)
    J = numpy.stack([P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]], axis=2)
    Jinv = numpy.linalg.inv(J)
    ref = numpy.einsum('mrd,mqd->mqr', Jinv, X - P[:, None, 0])
    m, nq = X.shape[:2]
    g = reference.tabulate_grad(V.degree, ref.reshape(-1, 2)).reshape(m, nq, -1, 2)
    Uc = U[:, V.layout.cell_dofs[cells]]                        # (dim, m, nloc)
    gref = numpy.einsum('kmj,mqjr->kmqr', Uc, g)
    return numpy.einsum('mrd,kmqr->kmqd', Jinv, gref)


def indicator(u, npoints=3):
    '''eta2 (nc,) of the Function u.'''
    V = u.function_space()
    mesh = V.mesh()
    U = u.array().reshape(V.dim, V.N)
    inner, pairs = edge_cells(mesh)
    ev = mesh.edges[inner]
    a, b = mesh.points[ev[:, 0]], mesh.points[ev[:, 1]]
    x, w = numpy.polynomial.legendre.leggauss(npoints)
    s = 0.5 * (x + 1.0)
    X = a[:, None, :] + s[None, :, None] * (b - a)[:, None, :]
    length = numpy.hypot(*(b - a).T)
    t = (b - a) / length[:, None]
    nrm = numpy.stack([t[:, 1], -t[:, 0]], axis=1)
    jump = _gradients(V, U, pairs[:, 0], X) - _gradients(V, U, pairs[:, 1], X)
    jn = numpy.einsum('kmqd,md->kmq', jump, nrm)
    integral = length * numpy.einsum('kmq,q->m', jn**2, 0.5 * w)
    term = length / 24.0 * integral
    eta2 = numpy.zeros(mesh.num_cells())
    numpy.add.at(eta2, pairs[:, 0], term)
    numpy.add.at(eta2, pairs[:, 1], term)
    return eta2


# -- fields with known indicators ---------------------------------------------
DIAGONALS = ('right', 'left', 'left/right', 'right/left', 'crossed')


def field(V, funcs):
    from flow_amd import fem
    u = fem.Function(V)
    xy = V.layout.dof_coords
    u.set_array(numpy.concatenate([f(xy[:, 0], xy[:, 1]) for f in funcs]))
    return u


def kink_expectation(mesh):
    '''eta2 of u = |x - 1/2| on a mesh with a line of edges at x = 1/2: each
    such edge gives |E|^2 / 6 to both of its cells (a jump of 2: |E| / 24 *
    4 |E|).'''
    p = mesh.points[mesh.edges]
    on = (p[:, 0, 0] == 0.5) & (p[:, 1, 0] == 0.5)
    length = numpy.hypot(*(p[:, 0] - p[:, 1]).T)
    want = numpy.zeros(mesh.num_cells())
    inner = numpy.zeros(mesh.num_edges(), dtype=bool)
    inner[edge_cells(mesh)[0]] = True
    for k in range(3):
        e = mesh.cell_edges[:, k]
        want += numpy.where(on[e] & inner[e], length[e]**2 / 6.0, 0.0)
    return want


# (degree, components, functions, max |grad u|) of global polynomials
SMOOTH = [
    (2, 1, [lambda x, y: 1 + 2 * x - 3 * y + 0.5 * x * x + x * y - 2 * y * y], 9.0),
    (1, 1, [lambda x, y: 3 + x - 2 * y], 2.0),
    (2, 1, [lambda x, y: 3 + x - 2 * y], 2.0),
    (2, 2, [lambda x, y: 3 + x - 2 * y, lambda x, y: x * x - y * x], 3.0),
    ]


# -- the adaptive Poisson problem ---------------------------------------------
SIGMA, FRACTION, CYCLES = 0.05, 0.5, 6
CENTRE = (0.5, 0.5)


def bump(x, y, sigma=SIGMA):
    r2 = (x - CENTRE[0])**2 + (y - CENTRE[1])**2
    return numpy.exp(-r2 / (2.0 * sigma**2))


def bump_code(sigma=SIGMA):
    '''(u, -laplace u) of the Gaussian bump as Expression code.'''
    r2 = '(pow(x[0] - %r, 2) + pow(x[1] - %r, 2))' % CENTRE
    u = 'exp(-%s / %r)' % (r2, 2.0 * sigma**2)
    f = '(%r - %s / %r) * %s' % (2.0 / sigma**2, r2, sigma**4, u)
    return u, f


def l2_error(V, values, sigma=SIGMA):
    '''|| u_h - u ||_L2 of the P1 field `values` against the bump, by a
    degree-6 rule on every cell (host).'''
    mesh = V.mesh()
    pts, wts = reference.triangle_rule(6)
    P = mesh.points[mesh.cell_vertices]                         # (nc, 3, 2)
    L = numpy.stack([1.0 - pts[:, 0] - pts[:, 1], pts[:, 0], pts[:, 1]], axis=1)
    X = numpy.einsum('ql,cld->cqd', L, P)
    uh = numpy.einsum('ql,cl->cq', L, values[V.layout.cell_dofs])
    e = uh - bump(X[:, :, 0], X[:, :, 1], sigma)
    # (the rule's weights sum to 1/2: the integral is |det J| sum_q w_q f_q)
    return float(numpy.sqrt((e**2 * wts[None, :]).sum(axis=1)
                            .dot(2.0 * mesh.cell_areas())))


def uniform_error_for(ndofs, errors):
    '''The error of the coarsest uniform mesh of `errors` [(dofs, error)]
    with at least ndofs dofs.'''
    for n, e in errors:
        if n >= ndofs:
            return n, e
    raise AssertionError('no uniform mesh with %d dofs among %r'
                         % (ndofs, errors))


def poisson(mesh, sigma=SIGMA):
    '''(V, a, L, bcs) of -laplace u = f, P1, with the bump as the solution
    and as Dirichlet data.'''
    from flow_amd import fem
    from flow_amd.fem import TestFunction, TrialFunction, dx, grad, inner
    V = fem.FunctionSpace(mesh, 'CG', 1)
    ucode, fcode = bump_code(sigma)
    u, v = TrialFunction(V), TestFunction(V)
    a = inner(grad(u), grad(v)) * dx
    L = fem.Expression(fcode, degree=4) * v * dx
    bcs = [fem.DirichletBC(V, fem.Expression(ucode, degree=4), 'on_boundary')]
    return V, a, L, bcs


def host_solve(mesh, sigma=SIGMA):
    '''(V, nodal values) of the Poisson problem by the host evaluator's
    matrices (tests/bilinear_reference.py) and a sparse LU, with the rows
    and columns of the Dirichlet dofs eliminated as host_newton does.'''
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    from flow_amd import fem
    import bilinear_reference as bref
    V, a, L, bcs = poisson(mesh, sigma)
    dofs, g = fem.bcs.collect(list(bcs), V.N)
    keep = numpy.ones(V.N)
    keep[dofs] = 0.0
    x0 = numpy.zeros(V.N)
    x0[dofs] = g
    A = bref.matrix(a)
    K = sp.diags(keep)
    b = keep * (bref.vector(L) - A.dot(x0))
    Ah = K.dot(A).dot(K) + sp.diags(1.0 - keep)
    return V, x0 + spla.splu(Ah.tocsc()).solve(b)


def uniform_errors(solve, upto, mesh):
    '''[(dofs, error)] of `mesh` and its uniform refinements until one has
    at least `upto` dofs; solve(mesh) -> (V, nodal values).'''
    from flow_amd import fem
    out = []
    while True:
        V, x = solve(mesh)
        out.append((V.N, l2_error(V, x)))
        if V.N >= upto:
            return out
        mesh = fem.refine(mesh)
