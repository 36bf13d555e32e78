# -*- coding: utf-8 -*-
'''
Nullspaces ("Nullspaces"; fem.VectorSpaceBasis,
flow_deflate): what the projection costs and what it buys.

  deflate   flow_deflate (two launches, in place) against the composed
            sequence it replaces -- flow_multi_dot (two launches), a negation,
            flow_combine into a second buffer, a copy back -- with k = 1 on
            the pressure slice and k = 3 (the rigid-body modes) on the velocity
            space of the P2/P1 space of karman_channel(nx, ny, fitted=True)
            (default 1035 x 241): HIP events around `batch` calls back to
            back, 3 warm-ups, then 7 windows of each, the two ALTERNATING
            window by window in one process; medians with min - max, and the
            ratio.  The two results are compared bit for bit first.
  loops     mixed.minres and mixed.fgmres for a fixed number of iterations
            (they stop with NotConverged, which is caught) on the Stokes
            matrix of that space, with the plain and with the deflated
            preconditioner: a host clock with a synchronise over the whole
            loop, per iteration.  Host driven: an end-to-end figure.
  Picard    Kovasznay's flow at Re = 40 (tools/oseen_lab.py's loop: velocity
            Dirichlet on the whole boundary), once with the pressure pinned at
            a corner vertex (FixedDofsBC) and once with
            nullspace=constant_nullspace(WP): FGMRES iterations per step and
            the pressure error against the exact field, both taken up to
            their means.

    python tools/nullspace_lab.py [NX [NY]] [--iterations K] [--picard N] [--steps S]
'''
import argparse
import os
import sys

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from flow_amd import fem, device, _hip               # noqa: E402
from flow_amd.fem import (                           # noqa: E402
    TestFunctions, solve, dx, inner, mixed, nullspace, ops,
    )
from flow_amd.fem.bcs import FixedDofsBC             # noqa: E402
from mixed_form_lab import walled, problem           # noqa: E402
from oseen_lab import oseen, timed_alternating       # noqa: E402


def deflate_lab(ns, x, tag):
    '''flow_deflate against the composed five launches on the vector x.'''
    lib = _hip.lib()
    store, ld, work = ns._store()
    k, n = ns.dim(), ns.support[1]
    xs = ns._slice(x)
    coef, minus = device.empty(k), device.empty(k)
    tmp = device.empty(n)
    Zp = _hip.f64(store, (k - 1) * ld + n)

    def composed(v):
        _hip.check(lib.flow_multi_dot(n, k, Zp, ld, _hip.f64(v, n),
                                      _hip.f64(work), _hip.f64(coef, k),
                                      _hip.stream()))
        ops.axpby(-1.0, coef, 0.0, minus)
        _hip.check(lib.flow_combine(n, k, Zp, ld, 1, _hip.f64(minus, k),
                                    _hip.f64(v, n), _hip.f64(tmp, n), ld,
                                    _hip.stream()))
        ops.copy(v, tmp)

    a, b = xs.clone(), xs.clone()
    one = lambda: _hip.check(lib.flow_deflate(           # noqa: E731
        n, k, Zp, ld, _hip.f64(b, n), _hip.f64(work), None, _hip.stream()))
    composed(a)
    one()
    same = bool(torch.equal(a, b))
    print('%s: flow_deflate == composed bit for bit: %s' % (tag, same))
    assert same
    tc, td = timed_alternating([lambda: composed(a), one])
    print('%s (n = %d, k = %d)' % (tag, n, k))
    print('  composed (5 launches, a temporary): %8.4f ms (%.4f - %.4f)' % tc)
    print('  flow_deflate (2 launches):          %8.4f ms (%.4f - %.4f)' % td)
    print('  composed / flow_deflate:            %8.3f' % (tc[0] / td[0]))
    # the traffic model: both launches read Z and x, the second writes x
    gb = 8.0 * n * (2 * k + 3) / 1.0e9
    print('  model %.4f GB: %.0f GB/s' % (gb, gb / (td[0] * 1.0e-3)))


def loops_lab(nx, ny, iterations):
    mesh, WP, a, L, bcs = problem(nx, ny)
    W, P = WP.sub(0), WP.sub(1)
    print('karman_channel(%d, %d, fitted): %d cells, 2 x %d + %d = %d unknowns'
          % (nx, ny, mesh.num_cells(), W.N, P.N, WP.size()))
    rng = numpy.random.RandomState(0)
    x = device.to_device(rng.standard_normal(WP.size()))
    deflate_lab(fem.constant_nullspace(WP), x, 'pressure constant')
    deflate_lab(fem.rigid_body_modes(W), x[:W.size()].clone(),
                'rigid-body modes on the velocity space')
    ns = fem.constant_nullspace(WP)
    masks = {}
    A, b = mixed.assemble_system(a, L, bcs, None, masks)
    Mm = mixed.BlockPreconditioner(A, 'jacobi',
                                   mixed._schur_diagonal(A, masks['p']),
                                   masks['u'])
    Mg = mixed.BlockTriangularPreconditioner(
        A, 'ilu0', mixed._signed_schur_diagonal(A, masks['p']))
    for name, run in (
            ('MINRES jacobi', lambda prec, w: mixed.minres(
                A.apply, prec, b.data, w, 1.0e-30, maxit=iterations)),
            ('FGMRES ilu0', lambda prec, w: mixed.fgmres(
                A.apply_fused, prec, b.data, w, 1.0e-30, maxit=iterations,
                restart=iterations))):
        plain = Mm.apply if name.startswith('MINRES') else Mg.apply
        for what, prec in (('plain', plain), (
                'deflated', nullspace.deflated_preconditioner(ns, plain))):
            def loop():
                w = device.zeros(A.size)
                try:
                    run(prec, w)
                except _hip.NotConverged:
                    pass

            t = walled(loop)
            print('%-14s %-9s: %8.3f ms per iteration (%.3f - %.3f), %d '
                  'iterations per window'
                  % ((name, what) + tuple(v / iterations for v in t)
                     + (iterations,)))


def picard_lab(n, steps):
    re = 40.0
    lam = re / 2.0 - numpy.sqrt(re * re / 4.0 + 4.0 * numpy.pi ** 2)
    two_pi = 2.0 * numpy.pi
    mesh = fem.RectangleMesh(fem.Point(-0.5, -0.5), fem.Point(1.0, 1.5), n, n)
    WP = fem.FunctionSpace(
        mesh, fem.VectorElement('Lagrange', 'triangle', 2)
        * fem.FiniteElement('Lagrange', 'triangle', 1))
    W, P = WP.sub(0), WP.sub(1)
    ue = fem.Expression(
        ('1.0 - exp(lam*x[0])*cos(k*x[1])', 'lam/k*exp(lam*x[0])*sin(k*x[1])'),
        degree=4, lam=float(lam), k=float(two_pi))
    xp = P.layout.dof_coords
    exact_p = 0.5 * (1.0 - numpy.exp(2.0 * lam * xp[:, 0]))
    pin = int(numpy.abs(xp - [-0.5, -0.5]).sum(axis=1).argmin())
    velocity = [fem.DirichletBC(WP.sub(0), ue, 'on_boundary')]
    (v, q) = TestFunctions(WP)
    L = inner(fem.Constant((0.0, 0.0)), v) * dx
    n2 = W.size()
    prm = {'krylov_solver': {'restart': 400, 'maximum_iterations': 4000}}
    print('Kovasznay, Re = 40, RectangleMesh %d x %d, P2/P1: %d unknowns'
          % (n, n, WP.size()))
    for name, bcs, ns in (
            ('corner pin', velocity + [FixedDofsBC(
                WP.sub(1), [pin], exact_p[[pin]])], None),
            ('nullspace=', velocity, fem.constant_nullspace(WP))):
        w_old, w = fem.Function(WP), fem.Function(WP)
        a = oseen(WP, fem.Constant(1.0 / re), fem.split(w_old)[0])
        its, defect = [], 0.0
        for _ in range(steps):
            info = solve(a == L, w, bcs, solver_parameters=prm, nullspace=ns)
            its.append(info.iterations)
            defect = max(defect, info.rhs_defect or 0.0)
            w_old.set_array(w.array())
        ph = w.array()[n2:]
        err = numpy.abs((ph - ph.mean()) - (exact_p - exact_p.mean())).max() \
            / numpy.abs(exact_p - exact_p.mean()).max()
        print('  %-11s iterations per step %s (sum %d); pressure error up to '
              'the mean %.4e; largest rhs_defect %.2e'
              % (name, its, sum(its), err, defect))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('nx', nargs='?', type=int, default=1035)
    ap.add_argument('ny', nargs='?', type=int, default=None)
    ap.add_argument('--iterations', type=int, default=20)
    ap.add_argument('--picard', type=int, default=16,
                    help='cells per side of the Kovasznay mesh (0: skip)')
    ap.add_argument('--steps', type=int, default=12, help='Picard steps')
    args = ap.parse_args()
    ny = args.ny if args.ny is not None else int(round(args.nx * 509.0 / 2182.0))
    with fem.mixed_arguments(True), fem.vector_arguments(True), \
            fem.mixed_gmres(True):
        _hip.lib()
        if args.picard:
            picard_lab(args.picard, args.steps)
        if args.nx:
            loops_lab(args.nx, ny, args.iterations)


if __name__ == '__main__':
    main()
