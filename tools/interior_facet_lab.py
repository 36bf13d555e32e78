# -*- coding: utf-8 -*-
'''
Interior-facet integrals ("Interior facets"): what a dS
part costs, against the one formula that a kernel of its own computes too.

  kelly     eta2 = |E|/24 int_E [grad u . n]^2 per cell, twice: JumpIndicator
            (flow_jump_indicator, one lane per cell, every interior edge from
            both of its cells) and cell_indicator(FacetArea/24 *
            jump(grad(u), n)**2 * dS, share=1.0) (the interpreter, one lane per
            facet, then the cell gather).  Prints the largest difference and
            the time of each (HIP events, median of 7, min - max); the
            cell_indicator's time includes compiling the program on the host.
  flowrate  u[0]('+')*dS(k) over the interior edges nearest a cross-section
            of the channel: the value, the number of facets and the time of
            one assemble (wall clock: it reads the result back).

    python tools/interior_facet_lab.py [kelly|flowrate|all] [nx]
'''
import os
import sys
import time

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_amd import fem, device       # noqa: E402
from flow_amd.fem import (              # noqa: E402
    FacetArea, FacetNormal, JumpIndicator, Measure, MeshFunction, assemble,
    dS, grad, jump,
    )


def timed(call, warmup=2, repeat=7):
    for _ in range(warmup):
        call()
    device.synchronize()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), \
            torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return numpy.median(ms), min(ms), max(ms)


def _field(V):
    u = fem.Function(V)
    xy = V.layout.dof_coords
    u.set_array(numpy.sin(25 * xy[:, 0]) * xy[:, 1] + xy[:, 0]**2)
    return u


def kelly(nx):
    mesh = fem.karman_channel(nx, fitted=True)
    n = FacetNormal(mesh)
    print('kelly: %d cells, %d interior facets'
          % (mesh.num_cells(), len(mesh.interior_facets)))
    for degree in (1, 2):
        V = fem.FunctionSpace(mesh, 'CG', degree)
        u = _field(V)
        J = JumpIndicator(V)
        form = FacetArea(mesh) / 24 * jump(grad(u), n)**2 * dS
        a = device.to_host(J.apply(u)).numpy()
        b = device.to_host(fem.cell_indicator(form, share=1.0)).numpy()
        out = device.empty(mesh.num_cells())
        tj = timed(lambda: J.apply(u, out=out))
        tf = timed(lambda: fem.cell_indicator(form, share=1.0, out=out))
        print('  P%d  max |difference| / max eta2 %.2e | JumpIndicator %.3f ms '
              '(%.3f - %.3f) | cell_indicator %.3f ms (%.3f - %.3f)'
              % ((degree, numpy.abs(a - b).max() / a.max()) + tj + tf))


def flowrate(nx):
    mesh = fem.karman_channel(nx, fitted=True)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    u = fem.Function(W)
    xy = W.layout.dof_coords
    H = xy[:, 1].max()
    u.set_array(numpy.concatenate([4.0 * xy[:, 1] * (H - xy[:, 1]) / H**2,
                                   0.0 * xy[:, 0]]))
    # the vertical interior edges nearest x = 0.4
    p = mesh.points[mesh.edges]
    vertical = numpy.abs(p[:, 0, 0] - p[:, 1, 0]) < 1e-12
    xs = numpy.unique(p[vertical, 0, 0])
    x0 = xs[numpy.abs(xs - 0.4).argmin()]
    m = MeshFunction('size_t', mesh, 1, 0)
    m.set_where(vertical & (numpy.abs(p[:, 0, 0] - x0) < 1e-12), 1)
    dSm = Measure('dS', domain=mesh, subdomain_data=m)
    form = u[0]('+') * dSm(1)
    assemble(form)
    device.synchronize()
    t0 = time.perf_counter()
    q = assemble(form)
    ms = 1e3 * (time.perf_counter() - t0)
    count = fem.ops.interior_facet_lists(mesh, m, 1).count
    print('flowrate: x = %.4f, %d facets, Q = %.15g (2 H / 3 = %.15g), '
          'assemble %.3f ms' % (x0, count, q, 2.0 * H / 3.0, ms))


def main(argv):
    what = argv[1] if len(argv) > 1 else 'all'
    nx = int(argv[2]) if len(argv) > 2 else 240
    with fem.interior_facets(True):
        if what in ('kelly', 'all'):
            kelly(nx)
        if what in ('flowrate', 'all'):
            flowrate(nx)


if __name__ == '__main__':
    main(sys.argv)
