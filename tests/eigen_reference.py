# -*- coding: utf-8 -*-
'''
An independent restatement of fem.Eigenmodes in numpy / scipy: the smallest
eigenpairs of A x = lambda M x on the free dofs, by elimination -- the rows and
columns of the Dirichlet dofs are cut out of the host matrices (no identity
rows, hence no spurious unit eigenvalues) -- and a direct solve:
scipy.linalg.eigh on the dense matrices for small problems, scipy.sparse.
linalg.eigsh in shift-invert mode otherwise.  No code is shared with
flow_amd/fem/eigen.py.
'''
import numpy
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spla

DENSE_LIMIT = 1500


def eliminate(A, M, isbc):
    '''(A_ff, M_ff, free indices) of scipy matrices and a boolean mask.'''
    free = numpy.nonzero(~numpy.asarray(isbc, dtype=bool))[0]
    A = sp.csr_matrix(A)[free][:, free]
    M = sp.csr_matrix(M)[free][:, free]
    return 0.5 * (A + A.T), 0.5 * (M + M.T), free


def smallest(A, M, isbc, k, sigma=None):
    '''(values (k,) ascending, vectors (n, k) M-orthonormal, zero on the
    Dirichlet dofs).  sigma: the shift of eigsh (default: a little below
    zero, so that a singular A can be factorised).'''
    n = A.shape[0]
    Af, Mf, free = eliminate(A, M, isbc)
    nf = len(free)
    if nf <= DENSE_LIMIT or k >= nf - 1:
        lam, Z = scipy.linalg.eigh(Af.toarray(), Mf.toarray())
        lam, Z = lam[:k], Z[:, :k]
    else:
        if sigma is None:
            sigma = -1.0e-3 * abs(Af.diagonal()).max() / abs(Mf.diagonal()).max()
        lam, Z = spla.eigsh(Af.tocsc(), k=k, M=Mf.tocsc(), sigma=sigma,
                            which='LM', tol=1e-13)
        order = numpy.argsort(lam)
        lam, Z = lam[order], Z[:, order]
    X = numpy.zeros((n, k))
    X[free, :] = Z
    return lam, X


def mass_lambda_min(M, isbc):
    '''The smallest eigenvalue of the free-dof mass matrix.'''
    _, Mf, free = eliminate(M, M, isbc)
    if len(free) <= DENSE_LIMIT:
        return float(scipy.linalg.eigvalsh(Mf.toarray())[0])
    return float(spla.eigsh(Mf.tocsc(), k=1, sigma=0.0, which='LM',
                            return_eigenvectors=False)[0])


def principal_angle(X, Y, M):
    '''The largest principal angle (radians) between span X and span Y in the
    M inner product.'''
    def orth(Z):
        G = Z.T.dot(M.dot(Z))
        L = numpy.linalg.cholesky(0.5 * (G + G.T))
        return scipy.linalg.solve_triangular(L, Z.T, lower=True).T
    Qx, Qy = orth(X), orth(Y)
    # sin of the largest angle: the part of Qy outside span Qx
    D = Qy - Qx.dot(Qx.T.dot(M.dot(Qy)))
    s = numpy.sqrt(numpy.linalg.eigvalsh(D.T.dot(M.dot(D))).clip(0.0).max())
    return float(numpy.arcsin(min(1.0, s)))


def match_once(got, want, radius):
    '''Assign every got[j] its own want[i] with |got[j] - want[i]| <=
    radius[j] (both ascending: greedy in order is exact for intervals on a
    line); the list of i, or None where no such assignment exists.'''
    used, out = -1, []
    for g, r in zip(got, radius):
        pick = None
        for i in range(used + 1, len(want)):
            if abs(g - want[i]) <= r:
                pick = i
                break
        if pick is None:
            return None
        used = pick
        out.append(pick)
    return out
