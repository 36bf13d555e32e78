# -*- coding: utf-8 -*-
'''
Host models tests/test_nullspace_gpu.py and tests/test_nullspace_host.py
compare fem.VectorSpaceBasis, flow_deflate and solve(..., nullspace=ns) with
(numpy and scipy only):

    deflate / deflate_fsum   x - Z^T (Z x) in extended precision, two ways
                             (numpy.longdouble; math.fsum of exact products of
                             a split), and the rounding bound of the device's
                             fp64 chain;
    bordered_solve           sparse LU of [[A, Z^T], [Z, 0]]: the solution of
                             the singular A x = b - Z^T (Z b) with Z x = 0;
    newton                   the loop of tests/mixed_newton_reference.py with
                             that bordered LU in place of the plain one.

Z is a (k, n) array of rows throughout (a full-length basis: zero outside its
support).
'''
import math

import numpy
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import mixed_newton_reference as mref

EPS = 2.0 ** -52


def deflate(Z, x):
    '''(x - Z^T (Z x), Z x) in numpy.longdouble.'''
    Zl = numpy.asarray(Z, dtype=numpy.longdouble)
    xl = numpy.asarray(x, dtype=numpy.longdouble)
    c = Zl.dot(xl)
    return xl - c.dot(Zl), c


def _two_prod(a, b):
    '''a * b as an exact sum of two doubles (Dekker / Veltkamp split).'''
    p = a * b
    split = 134217729.0
    t = split * a
    ah = t - (t - a)
    al = a - ah
    t = split * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def deflate_fsum(Z, x):
    '''The same from exactly rounded sums (math.fsum over exact products): c_j
    is the correctly rounded Z_j . x, and x_i - sum_j c_j Z_ji is rounded once.
    Returns doubles.'''
    Z = numpy.asarray(Z, dtype=numpy.float64)
    x = numpy.asarray(x, dtype=numpy.float64)
    c = numpy.zeros(Z.shape[0])
    for j in range(Z.shape[0]):
        terms = []
        for a, b in zip(Z[j], x):
            terms.extend(_two_prod(float(a), float(b)))
        c[j] = math.fsum(terms)
    out = numpy.zeros(len(x))
    for i in range(len(x)):
        terms = [float(x[i])]
        for j in range(Z.shape[0]):
            terms.extend(_two_prod(-float(c[j]), float(Z[j, i])))
        out[i] = math.fsum(terms)
    return out, c


def deflate_bound(Z, x):
    '''Per entry, the rounding bound of the fp64 chain c_j = sum_i fma(Z_ji,
    x_i, .) (n roundings, any order), x_i = fma(-c_j, Z_ji, x_i) for j < k (k
    roundings): with S_j = sum_i |Z_ji| |x_i|,
        |error_i| <= (n + k) eps (|x_i| + sum_j S_j |Z_ji|)
    to first order in eps; 1 % is added for the higher orders.  The bound of
    c_j alone: n eps S_j.'''
    Z = numpy.abs(numpy.asarray(Z, dtype=numpy.float64))
    ax = numpy.abs(numpy.asarray(x, dtype=numpy.float64))
    k, n = Z.shape
    S = Z.dot(ax)
    return 1.01 * (n + k) * EPS * (ax + S.dot(Z)), 1.01 * n * EPS * S


def full_basis(ns, size):
    '''The (k, size) host rows of a fem.VectorSpaceBasis.'''
    Z = numpy.zeros((ns.dim(), size))
    off, n = ns.support
    Z[:, off:off + n] = ns.host()
    return Z


def bordered_solve(S, Z, b):
    '''(x, lambda, relative residual of the LU) of [[S, Z^T], [Z, 0]] [x;
    lambda] = [b; 0] by sparse LU: for S singular with left and right
    nullspace span(Z^T), Z orthonormal rows, x solves S x = b - Z^T (Z b) with
    Z x = 0, and lambda = Z b.'''
    S = sp.csr_matrix(S)
    Zs = sp.csr_matrix(numpy.asarray(Z, dtype=numpy.float64))
    k = Zs.shape[0]
    K = sp.bmat([[S, Zs.T], [Zs, None if k == 0 else sp.csr_matrix((k, k))]],
                format='csc')
    rhs = numpy.concatenate([b, numpy.zeros(k)])
    sol = spla.splu(K).solve(rhs)
    res = numpy.linalg.norm(K.dot(sol) - rhs) / max(
        numpy.linalg.norm(rhs), numpy.finfo(float).tiny)
    n = S.shape[0]
    return sol[:n], sol[n:], res


def newton(F, J_hand, w, bcs, Z, relaxation=1.0, rtol=1.0e-9, atol=1.0e-10,
           maxit=50):
    '''mixed_newton_reference.newton with J delta = F solved by bordered_solve
    against the rows Z.  Returns (iterates, residuals, worst LU residual).'''
    from flow_amd.fem import assemble_system
    x = mref.start(w, bcs)
    iterates, residuals, worst = [x.copy()], [], 0.0
    while True:
        b = mref.residual(F, w, bcs)
        r = numpy.linalg.norm(b)
        residuals.append(r)
        if r < atol or r / residuals[0] < rtol or len(iterates) > maxit:
            return iterates, residuals, worst
        A, _ = assemble_system(J_hand, None, bcs)
        delta, _, res = bordered_solve(A.to_scipy(), Z, b)
        worst = max(worst, res)
        x = x - relaxation * delta
        w.set_array(x)
        iterates.append(x.copy())
