# -*- coding: utf-8 -*-
'''
Distributions along the boundary: the pressure coefficient Cp(theta) round
the cylinder, the wall shear tau_w(s) with its separation points, the local
heat flux along the heater -- any argument-free expression that is legal
under `ds`, evaluated at sample points of the wall facets instead of being
integrated to one number.

    P = BoundaryProfile(mesh, where='on_boundary', degree=2, start=None)
    P.evaluate(expr, out=None)  # device (ncomp, npoints), curve order
    P.integrate(expr)           # device (ncomp, nfacets): per-facet integrals
    P.cumulative(expr)          # device (ncomp, nfacets): running integral
    P.total(expr)               # device (ncomp, num_curves)
    P.crossings(values, level)  # host: arclengths of the sign changes
    P.angle(center)             # host: atan2 of the samples about center

where:

    'on_boundary'       every exterior facet;
    a SubDomain         the exterior facets it marks, by DirichletBC's rule
                        (inside(x, True) at both vertices and the mid point);
    (markers, id)       the exterior facets with markers == id, markers a
                        MeshFunction('size_t', mesh, 1) / FacetFunction, as
                        ds(id) reads it.

Curves (host, numpy, once).  The selected facets are chained by shared
vertices into boundary curves and every curve is traversed with the domain on
its left, along t = (-n_y, n_x), n the outward normal: the outer boundary
runs counter-clockwise, a hole clockwise.  A closed curve begins at its
lexicographically smallest vertex (x, then y); with start=(x, y) the closed
curve that holds the selected vertex nearest `start` begins at that vertex
(an open curve cannot be rotated and ignores it).  An open curve -- a marked
part of the boundary -- begins at the end from which t points along it.  The
curves are ordered by their first vertex, lexicographically.  A vertex that
more than two selected facets share (a bow-tie) is a ValueError; an empty
selection gives zero curves, and every method then returns empty arrays and
launches nothing.

Samples.  The m Gauss-Legendre points of reference.line_rule(degree) on every
facet, in the order of the traversal: npoints = m * nfacets, none at a vertex
(a gradient has two values there).  Host arrays, all in curve order:

    num_curves, closed (num_curves,), curve_facets (num_curves + 1,) offsets
    facet_index         position of the facet in mesh.bfacets
    facet_cell, facet_local, facet_length, facet_flip, normal (2, nfacets)
    s (npoints,)        arclength of the sample from its curve's start
    x (2, npoints)      sample coordinates
    weights (npoints,)  w_j * length: sum(values * weights) over a facet's
                        samples is its integral
    npoints, nfacets, m

Evaluation (flow_form_facet_values, csrc/form_kernels.hip): the facet
interpreter of assemble(f*ds), one lane per (facet, sample); the trace is
one-sided, from the cell that owns the facet.  One launch per group of two
components.  The facet lists are uploaded by the first call, rule and tables
are cached as those of the integrals; nothing is uploaded afterwards and
nothing synchronises.  The profile follows the boundary POLYGON (cells are
affine).  Not on strips.
'''
import numpy

from . import reference


def _no_strips():
    from .ops import _no_strips as refuse
    refuse('BoundaryProfile')


def selected_facets(mesh, where):
    '''Positions in mesh.bfacets of the facets `where` selects, ascending.'''
    from .bcs import facet_marked
    from .mesh import MeshFunction
    bf = mesh.bfacets
    if isinstance(where, str) or hasattr(where, 'inside'):
        if isinstance(where, str) and where != 'on_boundary':
            raise ValueError("where: %r; the only string is 'on_boundary'"
                             % (where,))
        return numpy.nonzero(facet_marked(where, mesh, bf, True))[0]
    if isinstance(where, tuple) and len(where) == 2 \
            and isinstance(where[0], MeshFunction):
        markers, value = where
        if markers.mesh is not mesh:
            raise ValueError('where: the facet markers belong to another mesh')
        return numpy.nonzero(markers.array()[bf] == value)[0]
    raise ValueError("where: 'on_boundary', a SubDomain or a pair (facet "
                     'markers, id)')


def _lexmin(points):
    '''Index of the lexicographically smallest row (x, then y).'''
    return int(numpy.lexsort((points[:, 1], points[:, 0]))[0])


def build_curves(mesh, sel, start=None):
    '''Chains the boundary facets at positions `sel` of mesh.bfacets into
    curves (the module's text).  Returns (order, flip, offsets, closed):
    `order` the entries of sel in curve order, flip[k] whether curve facet k is
    traversed against its own direction (reference.FACET_VERTICES), offsets
    (num_curves + 1,), closed (num_curves,).'''
    sel = numpy.asarray(sel, dtype=numpy.int64)
    nf = len(sel)
    if nf == 0:
        return (sel, numpy.zeros(0, dtype=bool), numpy.zeros(1, dtype=numpy.int64),
                numpy.zeros(0, dtype=bool))
    P = mesh.points
    local = mesh.bfacet_local[sel].astype(numpy.int64)
    cv = mesh.cell_vertices[mesh.bfacet_cell[sel]].astype(numpy.int64)
    fv = numpy.array(reference.FACET_VERTICES)
    rows = numpy.arange(nf)
    v0, v1, v2 = cv[rows, fv[local, 0]], cv[rows, fv[local, 1]], cv[rows, local]
    e = P[v1] - P[v0]
    # the outward normal points away from the cell's third vertex, the
    # traversal runs along t = (-n_y, n_x)
    nrm = numpy.stack([e[:, 1], -e[:, 0]], axis=1)
    inward = numpy.einsum('fd,fd->f', nrm, P[v2] - P[v0]) > 0.0
    nrm[inward] *= -1.0
    flip = (-nrm[:, 1] * e[:, 0] + nrm[:, 0] * e[:, 1]) < 0.0
    head = numpy.where(flip, v1, v0)
    tail = numpy.where(flip, v0, v1)
    count = numpy.bincount(numpy.concatenate([head, tail]))
    if count.max() > 2:
        v = int(count.argmax())
        raise ValueError(
            'the vertex (%r, %r) is shared by %d selected facets: the boundary '
            'does not chain into curves there'
            % (P[v, 0], P[v, 1], count[v]))
    out_of, in_of = {}, {}
    for f in range(nf):
        if int(head[f]) in out_of or int(tail[f]) in in_of:
            v = int(head[f]) if int(head[f]) in out_of else int(tail[f])
            raise ValueError(
                'the two selected facets at the vertex (%r, %r) do not follow '
                'one another' % (P[v, 0], P[v, 1]))
        out_of[int(head[f])] = f
        in_of[int(tail[f])] = f
    nearest = None
    if start is not None:
        start = numpy.asarray(start, dtype=numpy.float64).reshape(-1)
        if start.shape != (2,):
            raise ValueError('start: a point (x, y)')
        verts = numpy.unique(numpy.concatenate([head, tail]))
        verts = verts[numpy.lexsort((P[verts, 1], P[verts, 0]))]
        d = numpy.hypot(P[verts, 0] - start[0], P[verts, 1] - start[1])
        nearest = int(verts[int(d.argmin())])
    seen = numpy.zeros(nf, dtype=bool)
    curves = []                                    # (facets, closed)
    for f in range(nf):                            # open curves
        if int(head[f]) in in_of:
            continue
        chain = []
        while f is not None and not seen[f]:
            seen[f] = True
            chain.append(f)
            f = out_of.get(int(tail[f]))
        curves.append((chain, False))
    for f in range(nf):                            # what is left: closed ones
        if seen[f]:
            continue
        chain = []
        while not seen[f]:
            seen[f] = True
            chain.append(f)
            f = out_of[int(tail[f])]
        heads = head[chain]
        if nearest is not None and nearest in heads:
            first = int(numpy.nonzero(heads == nearest)[0][0])
        else:
            first = _lexmin(P[heads])
        curves.append((chain[first:] + chain[:first], True))
    firsts = numpy.array([P[head[c[0]]] for c, _ in curves])
    rank = numpy.lexsort((firsts[:, 1], firsts[:, 0]))
    curves = [curves[i] for i in rank]
    order = numpy.concatenate([numpy.array(c, dtype=numpy.int64)
                               for c, _ in curves])
    offsets = numpy.zeros(len(curves) + 1, dtype=numpy.int64)
    numpy.cumsum([len(c) for c, _ in curves], out=offsets[1:])
    closed = numpy.array([cl for _, cl in curves], dtype=bool)
    return sel[order], flip[order], offsets, closed


class BoundaryProfile(object):
    '''Sample points along the boundary curves of `mesh` and the evaluation
    of form expressions there; see the module's text.'''

    def __init__(self, mesh, where='on_boundary', degree=2, start=None):
        from .. import _hip
        _no_strips()
        degree = int(degree)
        if degree < 0:
            raise ValueError('degree: %d' % degree)
        pts, wts = reference.line_rule(degree)
        m = len(pts)
        if 3 * m > _hip.FORM_MAX_POINTS:
            raise ValueError(
                'degree %d: %d samples per facet, a facet rule of %d rows; the '
                'limit is %d rows' % (degree, m, 3 * m, _hip.FORM_MAX_POINTS))
        self.mesh = mesh
        self.degree = degree
        self.m = m
        sel = selected_facets(mesh, where)
        index, flip, offsets, closed = build_curves(mesh, sel, start)
        nf = len(index)
        self.nfacets = nf
        self.npoints = nf * m
        self.num_curves = len(closed)
        self.closed = closed
        self.curve_facets = offsets
        self.facet_index = index
        self.facet_flip = flip
        self.facet_cell = mesh.bfacet_cell[index].astype(numpy.int32)
        self.facet_local = mesh.bfacet_local[index].astype(numpy.int32)
        P = mesh.points
        cv = mesh.cell_vertices[self.facet_cell].astype(numpy.int64)
        fv = numpy.array(reference.FACET_VERTICES)
        rows = numpy.arange(nf)
        loc = self.facet_local.astype(numpy.int64)
        a = P[cv[rows, fv[loc, 0]]].reshape(nf, 2)
        b = P[cv[rows, fv[loc, 1]]].reshape(nf, 2)
        e = b - a
        self.facet_length = numpy.hypot(e[:, 0], e[:, 1])
        # t runs from a to b unless flipped; n = (t_y, -t_x)
        sgn = numpy.where(flip, -1.0, 1.0)
        with numpy.errstate(invalid='ignore', divide='ignore'):
            t = e * (sgn / self.facet_length)[:, None]
        self.normal = numpy.stack([t[:, 1], -t[:, 0]]) if nf \
            else numpy.zeros((2, 0))
        # the kernel's sample j of a facet sits at a + pts[j] (b - a) and
        # lands at position m-1-j of a flipped facet
        dest = numpy.where(flip[:, None], m - 1 - numpy.arange(m)[None, :],
                           numpy.arange(m)[None, :])            # (nf, m)
        xs = a[:, None, :] * (1.0 - pts)[None, :, None] \
            + b[:, None, :] * pts[None, :, None]                # (nf, m, 2)
        frac = numpy.where(flip[:, None], 1.0 - pts[None, :], pts[None, :])
        before = numpy.zeros(nf)
        for c in range(self.num_curves):
            lo, hi = offsets[c], offsets[c + 1]
            before[lo:hi] = numpy.cumsum(self.facet_length[lo:hi]) \
                - self.facet_length[lo:hi]
        sv = before[:, None] + frac * self.facet_length[:, None]
        wv = wts[None, :] * self.facet_length[:, None]
        x = numpy.zeros((nf, m, 2))
        s = numpy.zeros((nf, m))
        w = numpy.zeros((nf, m))
        if nf:
            x[rows[:, None], dest] = xs
            s[rows[:, None], dest] = sv
            w[rows[:, None], dest] = wv
        self.x = numpy.ascontiguousarray(x.reshape(nf * m, 2).T)
        self.s = s.reshape(-1)
        self.weights = w.reshape(-1)
        self._dev = None
        self._work = None

    # -- host helpers ---------------------------------------------------------
    def curve_length(self, c):
        lo, hi = self.curve_facets[c], self.curve_facets[c + 1]
        return float(self.facet_length[lo:hi].sum())

    def curve_points(self, c):
        '''The slice of the samples of curve c.'''
        return slice(int(self.curve_facets[c]) * self.m,
                     int(self.curve_facets[c + 1]) * self.m)

    def angle(self, center):
        '''atan2(y - c_y, x - c_x) of every sample, (npoints,).'''
        cx, cy = float(center[0]), float(center[1])
        return numpy.arctan2(self.x[1] - cy, self.x[0] - cx)

    def crossings(self, values, level=0.0):
        '''Per curve, the arclengths (ascending) where values - level changes
        sign between consecutive samples, by linear interpolation; the pair
        (last, first) of a closed curve included.  A sample exactly equal to
        `level` counts once, at its own arclength.  values: one scalar row of
        evaluate(), (npoints,) or (1, npoints), device or host.  A device
        row is READ BACK: this synchronises.'''
        if hasattr(values, 'is_cuda'):
            from .. import device
            values = device.to_host(values).numpy()
        v = numpy.asarray(values, dtype=numpy.float64).reshape(-1)
        if v.shape != (self.npoints,):
            raise ValueError('values: %d entries, the profile has %d samples'
                             % (v.size, self.npoints))
        found = []
        for c in range(self.num_curves):
            pts = self.curve_points(c)
            d, s = v[pts] - float(level), self.s[pts]
            hit = [s[d == 0.0]]
            if self.closed[c] and d.size:
                L = self.curve_length(c)
                d = numpy.append(d, d[0])
                s = numpy.append(s, s[0] + L)
            i = numpy.nonzero(d[:-1] * d[1:] < 0.0)[0]
            at = s[i] + (s[i + 1] - s[i]) * (d[i] / (d[i] - d[i + 1]))
            if self.closed[c]:
                at = numpy.where(at >= L, at - L, at)
            hit.append(at)
            found.append(numpy.sort(numpy.concatenate(hit)))
        return found

    # -- the device side ------------------------------------------------------
    def _lists(self):
        '''Device int32 lists (cell, local, dest, flip) in boundary-facet
        order, uploaded once; dest[k] the facet's position in curve order.'''
        if self._dev is None:
            from .. import device
            perm = numpy.argsort(self.facet_index, kind='stable')
            if not numpy.array_equal(numpy.sort(perm),
                                     numpy.arange(self.nfacets)):
                raise ValueError('facet destinations: not a permutation')
            self._dev = tuple(
                device.to_device(numpy.ascontiguousarray(a, dtype=numpy.int32))
                for a in (self.facet_cell[perm], self.facet_local[perm], perm,
                          self.facet_flip[perm]))
        return self._dev

    def _programs(self, expr):
        '''(expression, [(first component, Program)]): two components per
        program, one where two do not fit the limits of flow_form.'''
        from . import forms
        expr = forms.as_form(expr)
        forms._join_mesh(expr.mesh, self.mesh)
        trees = expr.scalar_trees()
        if any(forms.has_leaf(t, 'arg') for t in trees):
            raise ValueError(
                'the expression holds a test or trial function: a profile '
                'evaluates argument-free expressions')
        progs = []
        for k in range(0, len(trees), 2):
            try:
                progs.append((k, forms.compile_trees(trees[k:k + 2],
                                                     facet=True)))
            except forms.ProgramLimit:
                if len(trees[k:k + 2]) == 1:
                    raise
                for i in (k, k + 1):
                    progs.append((i, forms.compile_trees([trees[i]],
                                                         facet=True)))
        return len(trees), progs

    def _run(self, expr, values, integrals):
        '''Launches the programs of expr; values (ncomp, npoints) and
        integrals (ncomp, nfacets) or None, device.'''
        import ctypes
        from .. import _hip
        from .ops import _form_struct, mesh_struct
        ncomp, progs = expr
        lib = _hip.lib()
        cell, local, dest, flip = self._lists()
        nf, npts = self.nfacets, self.npoints
        vbase = _hip.f64(values, ncomp * npts, 'values').value
        ibase = None if integrals is None else \
            _hip.f64(integrals, ncomp * nf, 'integrals').value
        for k, prog in progs:
            fs, keep = _form_struct(prog, self.mesh, self.degree, facet=True)
            _hip.check(lib.flow_form_facet_values(
                ctypes.byref(mesh_struct(self.mesh)), ctypes.byref(fs), nf,
                _hip.i32(cell, nf, 'facet cells'),
                _hip.i32(local, nf, 'facet local indices'),
                _hip.i32(dest, nf, 'facet destinations'),
                _hip.i32(flip, nf, 'facet flips'),
                ctypes.c_void_p(vbase + 8 * k * npts),
                None if ibase is None else ctypes.c_void_p(ibase + 8 * k * nf),
                _hip.stream()))
            del keep

    @staticmethod
    def _array(rows, cols):
        from .. import device
        return device.empty(max(rows * cols, 1))[:rows * cols].view(rows, cols)

    def evaluate(self, expr, out=None):
        '''expr at the samples: a device fp64 tensor (ncomp, npoints) in curve
        order (ncomp = 1 for a scalar, 2 for a vector, 4 for a tensor, row
        major), written into `out` if given.  Enqueued on the package's
        stream; no host synchronisation.'''
        _no_strips()
        compiled = self._programs(expr)
        ncomp = compiled[0]
        if out is None:
            out = self._array(ncomp, self.npoints)
        elif tuple(out.shape) != (ncomp, self.npoints):
            raise ValueError('out: shape %r, the values have shape %r'
                             % (tuple(out.shape), (ncomp, self.npoints)))
        if self.npoints:
            self._run(compiled, out, None)
        return out

    def integrate(self, expr):
        '''The integral of expr over every facet, device (ncomp, nfacets) in
        curve order, by the rule of the samples: the per-facet values
        assemble(expr*ds) adds up at quadrature_degree = degree.'''
        _no_strips()
        compiled = self._programs(expr)
        ncomp = compiled[0]
        out = self._array(ncomp, self.nfacets)
        if self.nfacets:
            if self._work is None or self._work.numel() < ncomp * self.npoints:
                self._work = self._array(ncomp, self.npoints).view(-1)
            self._run(compiled, self._work, out)
        return out

    def cumulative(self, expr):
        '''The running integral of expr along each curve, device (ncomp,
        nfacets): entry k is the sum over the curve's facets 0..k, added
        strictly left to right (numpy.cumsum of integrate() per curve gives
        the same bits); the sum restarts at every curve.'''
        import ctypes
        from .. import _hip
        parts = self.integrate(expr)
        ncomp = parts.shape[0]
        out = self._array(ncomp, self.nfacets)
        if self.nfacets:
            offsets = (ctypes.c_int * (self.num_curves + 1))(
                *[int(o) for o in self.curve_facets])
            _hip.check(_hip.lib().flow_profile_cumsum(
                self.num_curves, offsets, ncomp, self.nfacets,
                _hip.f64(parts, ncomp * self.nfacets, 'integrals'),
                _hip.f64(out, ncomp * self.nfacets, 'out'), _hip.stream()))
        return out

    def total(self, expr):
        '''The integral of expr over each curve, device (ncomp, num_curves):
        the last entries of cumulative().'''
        import torch
        running = self.cumulative(expr)
        if self.num_curves == 0:
            return running[:, :0]
        if getattr(self, '_last', None) is None:
            self._last = torch.as_tensor(
                self.curve_facets[1:] - 1, dtype=torch.int64).to(running.device)
        return running.index_select(1, self._last)


# -- expression builders ----------------------------------------------------------
def _normal_of(f):
    from . import forms
    mesh = forms.as_form(f).mesh
    if mesh is None:
        raise ValueError('the field carries no mesh')
    return forms.FacetNormal(mesh)


def _stress_normal(u, n):
    '''(grad u + grad u^T) n, the two components.'''
    from . import forms
    gu = forms.grad(u)                          # gu[a, b] = d u_a / d x_b
    return [(gu[a, 0] + gu[0, a]) * n[0] + (gu[a, 1] + gu[1, a]) * n[1]
            for a in range(2)]


def traction(u, p, mu):
    '''-(mu (grad u + grad u^T) - p I) n, n the outward normal of the fluid:
    the force per length the fluid exerts on the wall, the integrand of
    KarmanProblem.forces() (its integral over the obstacle is (drag, lift)).'''
    from . import forms
    n = _normal_of(u)
    sn = _stress_normal(u, n)
    return forms.as_vector([-(mu * sn[a] - p * n[a]) for a in range(2)])


def wall_shear(u, mu):
    '''mu t . (grad u + grad u^T) n with t = (-n_y, n_x), the direction of the
    traversal: its zeros along a no-slip wall are the separation and
    reattachment points (BoundaryProfile.crossings).'''
    n = _normal_of(u)
    sn = _stress_normal(u, n)
    return mu * (sn[1] * n[0] - sn[0] * n[1])


def pressure_coefficient(p, p_ref, rho, U):
    '''(p - p_ref) / (rho U^2 / 2).'''
    return (p - p_ref) / (0.5 * rho * U * U)


def normal_flux(theta, kappa):
    '''-kappa grad(theta) . n, the heat flux out of the domain; kappa a
    number, a Constant, a field or an expression of them (a coefficient of
    flow_amd/materials.py at theta, for one).'''
    from . import forms
    n = _normal_of(theta)
    return -(kappa * forms.dot(forms.grad(theta), n))
