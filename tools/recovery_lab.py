# -*- coding: utf-8 -*-
'''
Gradient recovery and the ZZ indicator ("Recovered
gradients"): what the two launches cost and how good the estimate is.

On UnitSquareMesh(n, n), for P1 and P2, scalar and 2-vector, with the
interpolant of the manufactured solution u = sin(pi x) sin(pi y) (second
component: cos(pi x) sin(2 pi y)):

  recover ms     fem.GradientRecovery.apply(u, out=G): one launch of
                 flow_recover_gradient (HIP events around 20 calls back to
                 back, 3 warm-ups, median of 7 such windows with min - max);
  zz ms          flow_zz_indicator alone on the recovered gradient, the same
                 way; GB/s by the traffic model of DESIGN.md for both;
  effectivity    R.estimate(u) / |grad(u - u_exact)|_L2, the latter by a
                 form of degree 8 with the exact gradient evaluated at the
                 rule's points;
  recovered      |G - grad u_exact|_L2 / |grad(u_h - u_exact)|_L2.

    python tools/recovery_lab.py [n ...]        (default: 64 256 512)
'''
import ctypes
import math
import os
import sys

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_amd import fem, device, _hip       # noqa: E402
from flow_amd.fem import (                    # noqa: E402
    GradientRecovery, SpatialCoordinate, as_vector, assemble, cos, dx, grad,
    inner, sin,
    )
from flow_amd.fem.ops import mesh_struct, space_struct       # noqa: E402
from flow_amd.fem.recovery import _rule_dev                  # noqa: E402


def timed(call, warmup=3, repeat=7, batch=20):
    '''ms per call: `batch` calls back to back between two events (one
    launch alone is a few microseconds: that would time the events), median,
    min and max of `repeat` such windows.'''
    for _ in range(warmup):
        call()
    device.synchronize()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), \
            torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / batch)
    return numpy.median(ms), min(ms), max(ms)


def fields(V):
    xy = V.layout.dof_coords
    x, y = xy[:, 0], xy[:, 1]
    vals = [numpy.sin(math.pi * x) * numpy.sin(math.pi * y),
            numpy.cos(math.pi * x) * numpy.sin(2 * math.pi * y)][:V.dim]
    u = fem.Function(V)
    u.set_array(numpy.concatenate(vals))
    return u


def exact_gradients(mesh, dim):
    X = SpatialCoordinate(mesh)
    pi = fem.pi
    rows = [as_vector([pi * cos(pi * X[0]) * sin(pi * X[1]),
                       pi * sin(pi * X[0]) * cos(pi * X[1])]),
            as_vector([-pi * sin(pi * X[0]) * sin(2 * pi * X[1]),
                       2 * pi * cos(pi * X[0]) * cos(2 * pi * X[1])])]
    return rows[:dim]


def traffic(V, nc):
    '''Bytes the two launches move at least (DESIGN.md's model): per node the
    row bounds, the row itself and the output; per patch cell its six
    coordinates, dof indices and values; per cell of the indicator its
    coordinates, dof indices, values, recovered values and eta2.'''
    nloc, dim, N = V.layout.nloc, V.dim, V.N
    recover = N * (8 + 16 * dim) + nloc * nc * (4 + 48 + 4 * nloc + 8 * nloc * dim)
    zz = nc * (48 + 4 * nloc + 8 * nloc * 3 * dim + 8)
    return recover, zz


def run(n):
    mesh = fem.UnitSquareMesh(n, n)
    nc = mesh.num_cells()
    par = {'quadrature_degree': 8}
    for deg in (1, 2):
        for dim in (1, 2):
            V = fem.FunctionSpace(mesh, 'CG', deg, dim=dim)
            u = fields(V)
            R = GradientRecovery(V)
            G = R.apply(u)
            rec = timed(lambda: R.apply(u, out=G))
            eta2 = R.indicator(u)
            work = R._scratch()
            rule, nq = _rule_dev(deg)
            lib = _hip.lib()

            def zz():
                _hip.check(lib.flow_zz_indicator(
                    ctypes.byref(mesh_struct(mesh)),
                    ctypes.byref(space_struct(V.layout)), dim,
                    _hip.f64(u.data), _hip.f64(work), nq, _hip.f64(rule),
                    _hip.f64(eta2), _hip.stream()))

            ind = timed(zz)
            est = R.estimate(u)
            Gs = [G] if dim == 1 else list(G)
            us = [u] if dim == 1 else list(u.split())
            raw2 = rec2 = 0.0
            for uk, Gk, ge in zip(us, Gs, exact_gradients(mesh, dim)):
                raw2 += assemble(inner(grad(uk) - ge, grad(uk) - ge) * dx, par)
                rec2 += assemble(inner(Gk - ge, Gk - ge) * dx, par)
            b_rec, b_zz = traffic(V, nc)
            print('n %5d P%d x%d: %9d nodes %9d cells | recover %8.4f ms '
                  '(%.4f - %.4f) %7.1f GB/s | zz %8.4f ms (%.4f - %.4f) '
                  '%7.1f GB/s | effectivity %.4f | recovered / raw error %.4f'
                  % (n, deg, dim, V.N, nc, rec[0], rec[1], rec[2],
                     b_rec / rec[0] * 1e-6, ind[0], ind[1], ind[2],
                     b_zz / ind[0] * 1e-6, est / math.sqrt(raw2),
                     math.sqrt(rec2 / raw2)), flush=True)


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [64, 256, 512]
    for n in sizes:
        run(n)


if __name__ == '__main__':
    main()
