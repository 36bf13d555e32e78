# -*- coding: utf-8 -*-
'''
Cost of one (J, F) assembly of a Newton iteration: flow_form_newton (one
kernel, two gathers) against flow_form_matrix + flow_form_vector with the
separately compiled programs, on the bench mesh.  HIP
events, 2 warm-up calls, median of 7 with min and max; then one solve(F == 0)
of the P2 quasilinear problem, split into assembly, boundary conditions,
linear solve and norm (host clock around added synchronisations, not events:
the split costs a little).  The pair is ops.NewtonAssembler(fuse=False): the
untouched flow_form_matrix and flow_form_vector entry points with the
separately compiled programs (the cases here have one part, so no axpby is
added to either side).  Kernel-only times: run the script in a run of its own
under `rocprofv3 --kernel-trace` and read the durations of the form_* and
gather kernels, which are issued in the order printed here.

    python tools/newton_form_lab.py [nx [ny]] [--no-solve]
'''
import os
import sys
import time

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_amd import fem, materials, device          # noqa: E402
from flow_amd.fem import (                           # noqa: E402
    TestFunction, dx, inner, grad, derivative, ops,
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


def state(V, lo, hi):
    u = fem.Function(V)
    xy = V.layout.dof_coords
    u.set_array(lo + (hi - lo) * (0.5 + 0.5 * numpy.sin(9.0 * xy[:, 0])
                                  * numpy.cos(40.0 * xy[:, 1])))
    return u


def cases(V):
    v = TestFunction(V)
    u = state(V, 0.0, 1.0)
    yield 'quasilinear (1 + u^2)', u, (1 + u**2) * inner(grad(u), grad(v)) * dx
    th = state(V, 280.0, 340.0)
    yield 'heat kappa(theta)', th, materials.thermal_conductivity(th) \
        * inner(grad(th), grad(v)) * dx


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    nx = int(args[0]) if args else 2182
    ny = int(args[1]) if len(args) > 1 else int(round(nx * 509.0 / 2182.0))
    mesh = fem.karman_channel(nx, ny, fitted=True)
    print('mesh %d x %d: %d cells' % (nx, ny, mesh.num_cells()))
    for degree in (1, 2):
        V = fem.FunctionSpace(mesh, 'CG', degree)
        print('P%d: %d dofs, %d nonzeros' % (degree, V.N, V.layout.nnz))
        for name, u, F in cases(V):
            J = derivative(F, u)
            row = []
            for fuse in (True, False):
                asm = ops.NewtonAssembler(J, F, V, fuse=fuse)
                assert asm.fused == fuse
                row.append(timed(asm.assemble))
                lens = [len(j.program.code) for j in asm.jobs]
                print('  P%d %-22s %-6s %.3f ms (%.3f - %.3f)  programs %s'
                      % (degree, name, 'fused' if fuse else 'pair',
                         row[-1][0], row[-1][1], row[-1][2], lens))
            print('  P%d %-22s pair / fused = %.2f'
                  % (degree, name, row[1][0] / row[0][0]))
    if '--no-solve' in sys.argv:
        return
    # one solve, instrumented by wrapping the steps with synchronisations
    # (which the solve itself does not do: the split costs a little)
    V = fem.FunctionSpace(mesh, 'CG', 2)
    u = fem.Function(V)
    v = TestFunction(V)
    f = fem.Expression('100.0*sin(10.0*x[0])', degree=2)
    F = (1 + u**2) * inner(grad(u), grad(v)) * dx - f * v * dx
    bcs = [fem.DirichletBC(V, 0.0, 'on_boundary')]
    spent = {}

    def wrap(owner, name, label):
        inner_ = getattr(owner, name)

        def run(*a, **k):
            device.synchronize()
            t = time.perf_counter()
            out = inner_(*a, **k)
            device.synchronize()
            spent[label] = spent.get(label, 0.0) + time.perf_counter() - t
            return out
        setattr(owner, name, run)

    wrap(ops.NewtonAssembler, 'assemble', 'assembly')
    wrap(ops, 'symmetric_bc_matrix', 'boundary conditions')
    wrap(ops, 'krylov_solve', 'linear solve')
    wrap(ops, 'vector_norm', 'norm')
    t = time.perf_counter()
    from flow_amd import _hip
    try:
        info = fem.solve(F == 0, u, bcs, solver_parameters={
            'newton_solver': {'krylov_solver': {'relative_tolerance': 1e-8}}})
    except _hip.NotConverged as e:
        print('solve(F == 0), P2 quasilinear: NOT converged: %s' % e)
        for label, s in spent.items():
            print('  %-20s %.2f ms in all' % (label, 1e3 * s))
        return
    device.synchronize()
    total = time.perf_counter() - t
    print('solve(F == 0), P2 quasilinear: %r' % info)
    print('  residuals %s' % ['%.3e' % r for r in info.residuals])
    print('  linear iterations %s' % info.linear_iterations)
    n = max(info.iterations, 1)
    print('  total %.1f ms; per Newton iteration %.1f ms' % (
        1e3 * total, 1e3 * total / n))
    for label, s in spent.items():
        print('  %-20s %.2f ms per iteration' % (label, 1e3 * s / n))


if __name__ == '__main__':
    main()
