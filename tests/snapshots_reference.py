# -*- coding: utf-8 -*-
'''
Host restatement of flow_amd/fem/snapshots.py in numpy, independent of the
kernels, of ops.assemble_mass and of the Gram route the module takes:

    mass matrix   dense, summed from element matrices: the P1 / P2 basis of
                  tests/recovery_reference.py at Dunavant's 6-point rule
                  (exact to degree 4, the degree of a P2 x P2 product)
    lumped mass   |T| / 3 to every vertex of every cell
    POD           a dense SVD of L^T X, M = L L^T (Cholesky): no Gram matrix,
                  so no squared condition number
    DMD           the textbook SVD route on L^T X

A snapshot matrix X is (dim * N, k), component-blocked like Function.data.
'''
import numpy

import recovery_reference as rref


def mass_matrix(V):
    '''The consistent mass matrix of the scalar layout of V: dense (N, N).'''
    mesh = V.mesh()
    _, area = rref._geometry(mesh)
    phi = rref.basis(V.degree, rref.RULE_POINTS)                   # (nq, nloc)
    ref = numpy.einsum('q,qi,qj->ij', rref.RULE_WEIGHTS, phi, phi)
    cd = V.layout.cell_dofs
    M = numpy.zeros((V.N, V.N))
    numpy.add.at(M, (cd[:, :, None], cd[:, None, :]),
                 area[:, None, None] * ref[None])
    return M


def lumped_weights(V):
    '''The vertex-rule mass of a P1 space: (N,).'''
    assert V.degree == 1
    _, area = rref._geometry(V.mesh())
    w = numpy.zeros(V.N)
    numpy.add.at(w, V.layout.cell_dofs.ravel(), numpy.repeat(area / 3.0, 3))
    return w


def weight_matrix(V, inner):
    '''The scalar weight W (N, N) of `inner`, applied per component.'''
    if inner == 'L2':
        return mass_matrix(V)
    if inner == 'lumped':
        return numpy.diag(lumped_weights(V))
    assert inner == 'l2'
    return numpy.eye(V.N)


def weighted(V, W, X):
    '''W applied to every component of the columns of X (dim * N, k).'''
    N = V.N
    return numpy.concatenate([W.dot(X[c * N:(c + 1) * N])
                              for c in range(V.dim)], axis=0)


def gram(V, W, X):
    return X.T.dot(weighted(V, W, X))


def centre(X):
    return X - X.mean(axis=1, keepdims=True)


def pod_svd(X, L):
    '''POD of the columns of X in the inner product M = L L^T by a dense SVD
    of L^T X: (sigma (k,), modes (n, k) M-orthonormal, coefficients (k, k) =
    diag(sigma) V^T), so that X = modes @ coefficients.'''
    U, s, Vt = numpy.linalg.svd(L.T.dot(X), full_matrices=False)
    modes = numpy.linalg.solve(L.T, U)
    return s, modes, s[:, None] * Vt


def dmd_svd(X, L, r):
    '''Exact DMD of the sequence of columns of X, rank r, in the inner
    product M = L L^T: (eigenvalues (r,), modes (n, r) complex).'''
    Y = L.T.dot(X)
    Y0, Y1 = Y[:, :-1], Y[:, 1:]
    U, s, Vt = numpy.linalg.svd(Y0, full_matrices=False)
    U, s, Vh = U[:, :r], s[:r], Vt[:r].T
    At = U.T.dot(Y1).dot(Vh) / s
    lam, W = numpy.linalg.eig(At)
    modes = X[:, 1:].dot(Vh / s).dot(W) / lam
    return lam, modes


def subspace_gap(A, B, M):
    '''The distance between the spans of the M-orthonormal columns of A and B
    (equally many): the norm of (I - A A^T M) B, zero where they agree.'''
    MB = M.dot(B)
    R = B - A.dot(A.T.dot(MB))
    return numpy.sqrt(numpy.abs(numpy.einsum('ij,ij->j', R, M.dot(R))).max())


def match(got, want):
    '''got reordered so that got[i] is the entry nearest want[i] (greedy, for
    eigenvalue lists in no fixed order); the permutation.'''
    left = list(range(len(got)))
    perm = []
    for w in want:
        j = min(left, key=lambda i: abs(got[i] - w))
        perm.append(j)
        left.remove(j)
    return numpy.asarray(perm)
