# -*- coding: utf-8 -*-
'''
fem.Eigenmodes ("Eigenmodes"): what the two block kernels
cost against the per-column kernels they replace, timed in the same process.

On the P2 stiffness matrix of karman_channel(nx) (default nx = 1035: about
1.0 M rows, 11.6 M nonzeros):

  block product  Matrix.apply_block for m = 1, 2, 4, 8, 16 columns, with chunk
                 widths MC = 2, 4, 8 (LDS: MC * 8 KB per workgroup), against m
                 calls of flow_operator_apply.  Bytes moved per product in the
                 traffic model: 12 nnz (values and columns) once per launch,
                 4 (n + 1) row pointers, and per column 8 nnz gathered (mostly
                 from cache) plus 8 n written; the per-column path pays all of
                 it m times.
  block gram     flow_block_gram of ma x mb columns against mb calls of
                 flow_multi_dot; 8 n mb (ma + ceil(ma / 8)) bytes either way.

HIP events around `batch` calls back to back, 3 warm-ups, median of 7 such
windows with min - max.  At the default size the matrix (0.14 GB) stays in
the 256 MB Infinity Cache, for both sides of the comparison alike; --nx 2930
(7.9 M rows, a 1.1 GB matrix) is the HBM-resident size.

    python tools/eigen_lab.py [--nx NX]

--vector: the same for Eigenmodes on a vector space (fem.vector_eigenmodes).
The block product of the kind-2 matrix of P2 elasticity on karman_channel(nx)
(default nx = 730: 2N about 1.0 M rows, 5.6 M nonzeros in each of the four
value planes, 0.2 GB) for m = 1, 2, 3, 4, 8, 16 columns with MC = 2, 4 (LDS: MC
* 16 KB) against m calls of flow_operator_apply -- the table of DESIGN.md, from
which kBlockMC2 (csrc/eigen_kernels.hip) and DeviceBackend.BLOCK_FROM_2 are
read -- and a full solve, 'jacobi' against 'two_level', wall time.

    python tools/eigen_lab.py --vector [--nx NX] [--solve-nx NX]
'''
import argparse
import ctypes
import os
import sys

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_amd import fem, device, _hip       # noqa: E402
from flow_amd.fem import ops                 # noqa: E402


def timed(call, warmup=3, repeat=7, batch=10):
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


def product(nx):
    V = fem.FunctionSpace(fem.karman_channel(nx), 'P', 2)
    A = ops.assemble_stiffness(V)
    n, nnz = V.N, V.layout.nnz
    ld = n + (n & 1)
    mmax = 16
    print('P2 stiffness on karman_channel(%d): n = %d rows, %d nonzeros, %d '
          'row blocks' % (nx, n, nnz, A.operator().nblocks), flush=True)
    X = torch.rand(mmax * ld, dtype=torch.float64, device=device.get()) - 0.5
    Y = device.zeros(mmax * ld)
    Z = device.zeros(mmax * ld)

    def columns(m):
        for j in range(m):
            A.apply(X[j * ld:j * ld + n], Z[j * ld:j * ld + n])
    print('%3s %-10s %10s %22s %10s %8s' % ('m', 'path', 'ms', '(min - max)',
                                            'MB moved', 'ratio'))
    for m in (1, 2, 4, 8, 16):
        per_col = 12.0 * nnz + 4.0 * (n + 1) + 8.0 * nnz + 8.0 * n
        t0 = timed(lambda: columns(m))
        print('%3d %-10s %10.4f (%9.4f - %9.4f) %10.1f %8s'
              % (m, 'per column', t0[0], t0[1], t0[2], m * per_col * 1e-6, ''),
              flush=True)
        for mc in (2, 4, 8):
            nbytes = 12.0 * nnz + 4.0 * (n + 1) + m * (8.0 * nnz + 8.0 * n)
            t = timed(lambda: A.apply_block(X, ld, m, Y, ld, chunk=mc))
            print('%3d %-10s %10.4f (%9.4f - %9.4f) %10.1f %8.2f'
                  % (m, 'block MC %d' % mc, t[0], t[1], t[2], nbytes * 1e-6,
                     t0[0] / t[0]), flush=True)
            assert torch.equal(Y.view(mmax, ld)[:m, :n], Z.view(mmax, ld)[:m, :n])
    return n, ld, X, Y


def gram(n, ld, X, Y):
    lib = _hip.lib()
    st = _hip.stream()
    mmax = 16
    Y.copy_(torch.rand(mmax * ld, dtype=torch.float64, device=device.get()))
    work = device.empty(mmax * mmax * _hip.MULTI_DOT_BLOCKS)
    out = device.zeros(mmax * mmax)
    out2 = device.zeros(mmax * mmax)
    for ma, mb in ((8, 8), (16, 16), (16, 4)):
        nbytes = 8.0 * n * mb * (ma + -(-ma // 8))

        def block():
            _hip.check(lib.flow_block_gram(
                n, ma, _hip.f64(X), ld, mb, _hip.f64(Y), ld, _hip.f64(work),
                _hip.f64(out), st))

        def columns():
            for j in range(mb):
                _hip.check(lib.flow_multi_dot(
                    n, ma, _hip.f64(X), ld, _hip.f64(Y[j * ld:]),
                    _hip.f64(work), _hip.f64(out2[j * ma:]), st))
        t0 = timed(columns)
        t = timed(block)
        print('gram %2d x %2d: per column %8.4f ms (%.4f - %.4f), block %8.4f '
              'ms (%.4f - %.4f), ratio %.2f, %.1f MB, block %.0f GB/s'
              % (ma, mb, t0[0], t0[1], t0[2], t[0], t[1], t[2], t0[0] / t[0],
                 nbytes * 1e-6, nbytes / t[0] * 1e-6), flush=True)
        assert torch.equal(out[:ma * mb].view(ma, mb),
                           out2[:ma * mb].view(mb, ma).t())


def _elasticity(W, mu=1.0, lam=1.25):
    u, v = fem.TrialFunction(W), fem.TestFunction(W)
    eps = lambda w: fem.sym(fem.grad(w))                    # noqa: E731
    return (2 * mu * fem.inner(eps(u), eps(v))
            + lam * fem.div(u) * fem.div(v)) * fem.dx


def vector_product(nx):
    '''The block product of a kind-2 operator (P2 elasticity on karman_channel(
    nx): four value planes, columns of 2N) per MC and m against m applies.
    Traffic model: 36 nnz (four value planes and the columns) once per launch,
    4 (N + 1) row pointers, and per column 16 nnz gathered plus 16 N
    written.'''
    W = fem.VectorFunctionSpace(fem.karman_channel(nx), 'P', 2)
    A = fem.assemble(_elasticity(W))
    N, nnz = W.N, W.layout.nnz
    n = ld = 2 * N
    mmax = 16
    print('P2 elasticity on karman_channel(%d): N = %d, 2N = %d rows, %d '
          'nonzeros per plane, %d row blocks' % (nx, N, n, nnz,
                                                 A.operator().nblocks),
          flush=True)
    X = torch.rand(mmax * ld, dtype=torch.float64, device=device.get()) - 0.5
    Y = device.zeros(mmax * ld)
    Z = device.zeros(mmax * ld)

    def columns(m):
        for j in range(m):
            A.apply(X[j * ld:j * ld + n], Z[j * ld:j * ld + n])
    print('%3s %-10s %10s %22s %10s %8s' % ('m', 'path', 'ms', '(min - max)',
                                            'MB moved', 'ratio'))
    for m in (1, 2, 3, 4, 8, 16):
        per_col = 36.0 * nnz + 4.0 * (N + 1) + 16.0 * nnz + 16.0 * N
        t0 = timed(lambda: columns(m))
        print('%3d %-10s %10.4f (%9.4f - %9.4f) %10.1f %8s'
              % (m, 'per column', t0[0], t0[1], t0[2], m * per_col * 1e-6, ''),
              flush=True)
        for mc in (2, 4):
            nbytes = 36.0 * nnz + 4.0 * (N + 1) + m * (16.0 * nnz + 16.0 * N)
            t = timed(lambda: A.apply_block(X, ld, m, Y, ld, chunk=mc))
            print('%3d %-10s %10.4f (%9.4f - %9.4f) %10.1f %8.2f'
                  % (m, 'block MC %d' % mc, t[0], t[1], t[2], nbytes * 1e-6,
                     t0[0] / t[0]), flush=True)
            assert torch.equal(Y.view(mmax, ld)[:m, :n], Z.view(mmax, ld)[:m, :n])


def vector_solve(nx, k=6):
    '''A full solve, 'jacobi' against 'two_level': the k smallest vibration
    modes of a unit square of nx x nx cells (P2), clamped on its left edge.'''
    import time
    W = fem.VectorFunctionSpace(fem.UnitSquareMesh(nx, nx), 'P', 2)
    bc = fem.DirichletBC(W, (0.0, 0.0), lambda p, on: on and p[0] < 1e-10)
    E = fem.Eigenmodes(_elasticity(W), None, bc)
    print('P2 elasticity on UnitSquareMesh(%d, %d), clamped on x = 0: 2N = %d, '
          'k = %d, rtol 1e-8' % (nx, nx, 2 * W.N, k), flush=True)
    for pc in ('jacobi', 'two_level'):
        E.solve(k, maxit=2, preconditioner=pc, error_on_nonconvergence=False)
        device.synchronize()
        t = time.perf_counter()
        r = E.solve(k, maxit=2000, preconditioner=pc,
                    error_on_nonconvergence=False)
        device.synchronize()
        t = time.perf_counter() - t
        print('%-10s %5d iterations %9.3f s %8.2f ms / iteration  converged '
              '%d of %d  lambda_0 %.6f' % (pc, r.iterations, t,
                                           1e3 * t / max(r.iterations, 1),
                                           int(r.converged.sum()), k,
                                           r.values[0]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=None,
                    help='cells along the channel (default 1035; --vector: 730)')
    ap.add_argument('--vector', action='store_true',
                    help='the kind-2 block product and a solve on a vector '
                         'space (fem.vector_eigenmodes)')
    ap.add_argument('--solve-nx', type=int, default=96)
    args = ap.parse_args()
    if args.vector:
        with fem.vector_arguments(True), fem.vector_eigenmodes(True):
            vector_product(args.nx or 730)
            vector_solve(args.solve_nx)
        return
    n, ld, X, Y = product(args.nx or 1035)
    gram(n, ld, X, Y)


if __name__ == '__main__':
    main()
