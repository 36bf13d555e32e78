# -*- coding: utf-8 -*-
'''
numpy restatement of the tracer particles (flow_amd/fem/tracers.py), written
from the specification alone: the three explicit schemes, the loss rule and
the interpolation in time, on top of tests/point_reference.py.

  location   the lowest-index cell with min lambda >= -1e-12, by
             point_reference.locate.  Brute force over all cells for every
             stage of every substep is too slow to be a test, so `locate`
             here hands point_reference.locate the cells near each group of
             points only (coarse buckets of padded bounding boxes, ascending
             cell order kept: the answer is the brute force's, which
             tests/test_tracers_host.py asserts);
  velocity   `field_values`: the reference basis (reference.tabulate) at the
             barycentrics of point_reference.barycentric_own, all points at
             once -- point_reference.field_values without its loop over the
             points (asserted equal in the host test);
  schemes    euler, rk2 (midpoint), rk4 (classical);
  time       with u_next the velocity at fraction theta of the call's time
             steps * dt is (1 - theta) u + theta u_next, theta = (s + a) /
             steps for stage offset a in {0, 1/2, 1} of substep s;
  loss       a substep is accepted if all its stage points and its end point
             lie in some cell; else the particle keeps the position of the
             start of that substep, its cell becomes -1 and it is left alone.

`advect` also returns, per particle, the smallest distance of any of its
stage or end points (the failing one included) to the nearest boundary
facet: the particles whose fate rounding may decide.
'''
import numpy

from flow_amd.fem import reference

import point_reference as pref

SCHEMES = ('euler', 'rk2', 'rk4')


def diameter(mesh):
    '''Diagonal of the bounding box.'''
    p = mesh.points
    return float(numpy.linalg.norm(p.max(axis=0) - p.min(axis=0)))


# -- location -------------------------------------------------------------------
class _SubMesh(object):
    '''The cells `cells` (ascending) of a mesh, as point_reference.locate
    reads a mesh.'''

    def __init__(self, mesh, cells):
        self.points = mesh.points
        self.cells = cells
        self.cell_vertices = mesh.cell_vertices[cells]

    def num_cells(self):
        return len(self.cells)


class _Buckets(object):
    '''nb x nb buckets over the bounding box; a bucket lists, ascending,
    every cell whose bounding box, padded by 1e-6 of the domain, overlaps
    it.  A point that passes the cell test lies within ~1e-12 diameters of
    the cell, so inside the padded box, and the bucket index is monotone in
    the coordinates: the owner is among the bucket's cells.'''

    def __init__(self, mesh):
        p = mesh.points
        nc = mesh.num_cells()
        self.nb = nb = int(max(1, min(32, round(numpy.sqrt(nc / 24.0)))))
        self.lo = p.min(axis=0)
        ext = p.max(axis=0) - self.lo
        self.h = ext / nb
        v = p[mesh.cell_vertices]
        pad = 1.0e-6 * ext.max()
        i0 = self.index(v.min(axis=1) - pad)
        i1 = self.index(v.max(axis=1) + pad)
        self.sub = {}
        for ix in range(nb):
            for iy in range(nb):
                m = (i0[:, 0] <= ix) & (ix <= i1[:, 0]) \
                    & (i0[:, 1] <= iy) & (iy <= i1[:, 1])
                self.sub[ix, iy] = _SubMesh(mesh, numpy.nonzero(m)[0])

    def index(self, pts):
        t = numpy.floor((pts - self.lo) / self.h)
        t = numpy.nan_to_num(t, nan=0.0, posinf=self.nb, neginf=-1.0)
        return numpy.clip(t, 0, self.nb - 1).astype(numpy.int64)


_BUCKETS = []


def _buckets(mesh):
    for m, b in _BUCKETS:
        if m is mesh:
            return b
    b = _Buckets(mesh)
    _BUCKETS.append((mesh, b))
    if len(_BUCKETS) > 8:
        del _BUCKETS[0]
    return b


def locate(mesh, pts):
    '''point_reference.locate(mesh, pts), bucket by bucket.'''
    pts = numpy.asarray(pts, dtype=float).reshape(-1, 2)
    out = numpy.full(len(pts), -1, dtype=numpy.int32)
    if not len(pts):
        return out
    if len(pts) * mesh.num_cells() <= 200000:
        return pref.locate(mesh, pts)
    b = _buckets(mesh)
    idx = b.index(pts)
    key = idx[:, 0] * b.nb + idx[:, 1]
    order = numpy.argsort(key, kind='stable')
    bounds = numpy.nonzero(numpy.diff(key[order]))[0] + 1
    for grp in numpy.split(order, bounds):
        sub = b.sub[int(idx[grp[0], 0]), int(idx[grp[0], 1])]
        if not sub.num_cells():
            continue
        loc = pref.locate(sub, pts[grp])
        hit = loc >= 0
        out[grp[hit]] = sub.cells[loc[hit]]
    return out


# -- velocity -------------------------------------------------------------------
def field_values(u, pts, cells):
    '''Values of Function u at pts on their cells, (dim, n):
    point_reference.field_values, all points in one tabulate.'''
    V = u.function_space()
    lam = pref.barycentric_own(V.mesh(), pts, cells)
    U = u.array().reshape(V.dim, V.N)
    dofs = V.layout.cell_dofs[cells]                    # (n, nloc)
    tab = reference.tabulate(V.degree, lam[1:].T)       # (n, nloc)
    return numpy.einsum('dnj,nj->dn', U[:, dofs], tab)


def boundary_distance(mesh, pts):
    '''Distance of every point to the nearest boundary facet (a segment).'''
    seg = mesh.points[mesh.edges[mesh.bfacets]]         # (nf, 2, 2)
    a, d = seg[:, 0], seg[:, 1] - seg[:, 0]
    dd = (d * d).sum(axis=1)
    out = numpy.full(len(pts), numpy.inf)
    for s in range(0, len(pts), 4096):
        p = pts[s:s + 4096]
        w = p[:, None, :] - a[None, :, :]               # (n, nf, 2)
        t = numpy.clip((w * d[None]).sum(axis=2) / dd[None], 0.0, 1.0)
        r = w - t[:, :, None] * d[None]
        out[s:s + 4096] = numpy.sqrt((r * r).sum(axis=2)).min(axis=1)
    return numpy.where(numpy.isfinite(pts).all(axis=1), out, 0.0)


# -- the schemes ----------------------------------------------------------------
def advect(mesh, pts, u, dt, steps=1, scheme='rk4', u_next=None,
           distances=True):
    '''`steps` substeps for the particles that start at pts (n, 2).  Returns
    (positions (n, 2), cells (n,) int32 with -1 for the lost, dist (n,)):
    dist the smallest distance to the boundary over all the points the
    particle's substeps looked at (inf where none, or distances=False).'''
    assert scheme in SCHEMES
    pos = numpy.array(pts, dtype=float).reshape(-1, 2)
    n = len(pos)
    cells = locate(mesh, pos)
    dist = numpy.full(n, numpy.inf)

    def look(idx, x):
        '''cells of the points x of particles idx; records the distances'''
        if distances and len(idx):
            dist[idx] = numpy.minimum(dist[idx], boundary_distance(mesh, x))
        return locate(mesh, x)

    def velocity(x, c, theta):
        v = field_values(u, x, c)
        if u_next is not None:
            v = (1.0 - theta) * v + theta * field_values(u_next, x, c)
        return v.T                                       # (m, 2)

    live0 = numpy.nonzero(cells >= 0)[0]
    if distances and len(live0):
        dist[live0] = boundary_distance(mesh, pos[live0])
    for s in range(steps):
        idx = numpy.nonzero(cells >= 0)[0]
        if not len(idx):
            break
        x = pos[idx]
        ok = numpy.ones(len(idx), dtype=bool)
        th0, thm, th1 = s / steps, (s + 0.5) / steps, (s + 1.0) / steps

        def stage(xs, theta):
            '''velocity at the stage points of the particles still ok (zero
            rows for the others, which are lost already)'''
            k = numpy.zeros((len(idx), 2))
            act = numpy.nonzero(ok)[0]
            if len(act):
                c = look(idx[act], xs[act])
                good = c >= 0
                ok[act[~good]] = False
                act, c = act[good], c[good]
                if len(act):
                    k[act] = velocity(xs[act], c, theta)
            return k

        k1 = velocity(x, cells[idx], th0)
        if scheme == 'euler':
            end = x + dt * k1
        elif scheme == 'rk2':
            k2 = stage(x + 0.5 * dt * k1, thm)
            end = x + dt * k2
        else:
            k2 = stage(x + 0.5 * dt * k1, thm)
            k3 = stage(x + 0.5 * dt * k2, thm)
            k4 = stage(x + dt * k3, th1)
            end = x + (dt / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        act = numpy.nonzero(ok)[0]
        ce = numpy.full(len(idx), -1, dtype=numpy.int32)
        if len(act):
            ce[act] = look(idx[act], end[act])
        acc = ce >= 0
        pos[idx[acc]] = end[acc]
        cells[idx] = ce
    return pos, cells, dist


def taylor_matrix(scheme, dt):
    '''T_k(dt J), J = [[0, -1], [1, 0]]: one substep of the scheme on the
    rigid rotation u = J (x - c), the Taylor polynomial of exp of degree 1
    (euler), 2 (rk2) or 4 (rk4).'''
    J = numpy.array([[0.0, -1.0], [1.0, 0.0]])
    k = {'euler': 1, 'rk2': 2, 'rk4': 4}[scheme]
    T, P, f = numpy.eye(2), numpy.eye(2), 1.0
    for j in range(1, k + 1):
        P = P.dot(dt * J)
        f *= j
        T = T + P / f
    return T


# -- the cases the host and the GPU tests share ----------------------------------
def interpolate(V, funcs):
    from flow_amd import fem
    u = fem.Function(V)
    xy = V.layout.dof_coords
    u.set_array(numpy.concatenate(
        [f(xy[:, 0], xy[:, 1]) + 0.0 * xy[:, 0] for f in funcs]))
    return u


def rotation_case(kind):
    '''(mesh, centre, starts): circles that stay inside the mesh.'''
    from flow_amd import fem
    if kind == 'square':
        mesh = fem.UnitSquareMesh(12, 9)
        c = numpy.array([0.5, 0.5])
        radii = [0.05, 0.2, 0.35]
    else:
        mesh = fem.karman_channel(60, 14, fitted=True)
        # the hole (0.1, 0.01), radius 0.02, in the channel |y| <= 0.07:
        # circles about its centre lie between it and the walls for radii
        # in (0.02, 0.06); Euler's grow by 5.5 % over the run
        c = numpy.array(mesh.hole[:2], dtype=float)
        radii = [0.03, 0.04, 0.05]
    ang = numpy.array([0.3, 1.7, 2.9, 4.4, 5.6])
    starts = numpy.concatenate(
        [c + r * numpy.stack([numpy.cos(ang), numpy.sin(ang)], axis=1)
         for r in radii])
    return mesh, c, starts


def rotation_field(mesh, degree, c):
    '''u = (-(y - cy), x - cx): exact in P1 and P2.'''
    from flow_amd import fem
    V = fem.VectorFunctionSpace(mesh, 'CG', degree)
    return interpolate(V, [lambda x, y: -(y - c[1]), lambda x, y: x - c[0]])


def rotation_closed_form(c, starts, scheme, dt, steps):
    T = numpy.linalg.matrix_power(taylor_matrix(scheme, dt), steps)
    return c + (starts - c).dot(T.T)


ROTATION_STEPS = 120
ROTATION_DT = 0.03


def constant_field(mesh, degree, vx, vy=0.0):
    from flow_amd import fem
    V = fem.VectorFunctionSpace(mesh, 'CG', degree)
    return interpolate(V, [lambda x, y: vx + 0.0 * x, lambda x, y: vy + 0.0 * x])


EXIT_DT = 0.07
EXIT_STARTS = numpy.array([[x, y] for x in (0.105, 0.305, 0.505)
                           for y in (0.25, 0.6)])


def exit_prediction(steps):
    '''Uniform flow (1, 0) on the unit square, RK4, dt = EXIT_DT: a particle
    is lost at the first substep whose furthest stage point x + dt exceeds 1.
    (accepted substeps (n,), lost (n,), frozen or current positions).'''
    x0 = EXIT_STARTS[:, 0]
    most = numpy.floor((1.0 - x0) / EXIT_DT).astype(int)
    done = numpy.minimum(most, steps)
    pos = EXIT_STARTS.copy()
    pos[:, 0] = x0 + done * EXIT_DT
    return done, steps > most, pos


# fields that are not linear: the three meshes of the form tests
EPS = 2.2e-16
NONLINEAR_POINTS = 2000
NONLINEAR_STEPS = 20
EXCLUDE = 1.0e-6        # of the domain diameter
PERTURB = 1.0e-10       # of the domain diameter


def nonlinear_meshes():
    from flow_amd import fem
    return [fem.UnitSquareMesh(12, 9),
            fem.karman_channel(60, 14, fitted=True),
            fem.karman_channel_graded(lcar=1.0e-2)]


def nonlinear_case(mesh, k, degree):
    '''(u, u_next, dt, starts): smooth sin / cos velocities of speed ~1, the
    box's own lengths as wavelengths; 2000 random starts, a margin of 5 %
    outside the box (some start lost); dt such that 20 substeps carry a
    particle over about three cells.'''
    from flow_amd import fem
    lo, hi = mesh.points.min(axis=0), mesh.points.max(axis=0)
    ext = hi - lo
    V = fem.VectorFunctionSpace(mesh, 'CG', degree)

    def s(x, y):
        return 2.0 * numpy.pi * (x - lo[0]) / ext[0], \
            2.0 * numpy.pi * (y - lo[1]) / ext[1]

    def u0(x, y):
        a, b = s(x, y)
        return 1.0 + 0.4 * numpy.sin(a) * numpy.cos(b)

    def v0(x, y):
        a, b = s(x, y)
        return 0.25 * numpy.cos(2.0 * a + 0.5) * numpy.sin(b)

    def u1(x, y):
        a, b = s(x, y)
        return 0.8 + 0.3 * numpy.cos(a + 1.0) * numpy.cos(b)

    def v1(x, y):
        a, b = s(x, y)
        return -0.2 * numpy.sin(a) * numpy.sin(2.0 * b)

    u = interpolate(V, [u0, v0])
    u_next = interpolate(V, [u1, v1])
    h = numpy.sqrt(2.0 * ext[0] * ext[1] / mesh.num_cells())
    dt = 3.0 * h / (NONLINEAR_STEPS * 1.4)
    starts = pref.random_points(mesh, NONLINEAR_POINTS, seed=20 + k)
    return u, u_next, dt, starts


def nonlinear_reference(mesh, u, u_next, dt, starts):
    '''The restatement's run, the particles the comparison leaves out (a
    stage point within EXCLUDE diameters of the boundary: rounding may
    decide their fate) and the amplification A of the flow itself: starts
    moved by PERTURB diameters in a fixed direction, max |change of the end
    position| / that, over the particles alive in both runs, floored at 1.'''
    D = diameter(mesh)
    pos, cells, dist = advect(mesh, starts, u, dt, NONLINEAR_STEPS, 'rk4',
                              u_next=u_next)
    out = dist < EXCLUDE * D
    shift = PERTURB * D * numpy.array([0.6, 0.8])
    pos2, cells2, _ = advect(mesh, starts + shift, u, dt, NONLINEAR_STEPS,
                             'rk4', u_next=u_next, distances=False)
    both = (cells >= 0) & (cells2 >= 0) & ~out
    A = max(1.0, numpy.abs(pos2[both] - pos[both]).max() / (PERTURB * D))
    tol = 64.0 * EPS * 4 * NONLINEAR_STEPS * A * D
    return pos, cells, out, A, tol
