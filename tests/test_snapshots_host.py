# -*- coding: utf-8 -*-
'''
fem.Snapshots without a GPU (flow_amd/fem/snapshots.py): the host algebra
(pod_from_gram, dmd_from_gram) against the SVD restatement of tests/
snapshots_reference.py on explicit small matrices, rank truncation, centring,
the time-step rules, the refusals (all raised before the device is touched),
the bookkeeping of the store, the exports and the symbols.

The bound.  The method of snapshots works on G = X^T M X, whose rounding is
k eps lambda_1 and which an eigenvalue lambda_r sees magnified by lambda_1 /
lambda_r: every comparison below is held against

    c * k * eps * lambda_1 / lambda_r,    c = 5.

c comes from the restatement alone: its own Gram route in numpy (eigh of Y^T Y,
Y = L^T X) against its SVD route, on the matrices of this file, differs by
0.049 of that unit in the energies (relative to each energy), 0.049 in the
M-orthonormality of the modes, 0.011 in the subspaces and, for the DMD case,
0.022 in the eigenvalues (measured on the CPU); two orders of margin over the
largest, rounded up, give c = 5.  pod_from_gram / dmd_from_gram measured
against the SVD route: 0.027, 0.027, 0.0073 and 0.023 of the unit.
'''
import os

import numpy
import pytest

from flow_amd import fem

import snapshots_reference as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = numpy.finfo(float).eps
C_BOUND = 5.0
N, K = 40, 7
# sigma_1 / sigma_r = 1e3, one double singular value
SIGMA = numpy.array([1e3, 1e2, 1e2, 10.0, 5.0, 2.0, 1.0])
GROUPS = [[0], [1, 2], [3], [4], [5], [6]]


def _spd(rng, n):
    A = rng.randn(n, n)
    M = A.dot(A.T) / n + numpy.eye(n)
    return M, numpy.linalg.cholesky(M)


def _pod_case():
    '''X (40, 7) with the singular values SIGMA in the inner product M.'''
    rng = numpy.random.RandomState(7)
    M, L = _spd(rng, N)
    U, _ = numpy.linalg.qr(rng.randn(N, K))
    Vq, _ = numpy.linalg.qr(rng.randn(K, K))
    X = numpy.linalg.solve(L.T, U * SIGMA).dot(Vq.T)
    return X, M, L


def _dmd_case():
    '''Seven states of a linear map with the eigenvalues LAM on a
    four-dimensional invariant subspace (a decaying rotation and two decaying
    directions), amplitudes 30 : 1 : 1.'''
    rng = numpy.random.RandomState(3)
    M, L = _spd(rng, N)
    lam = numpy.array([0.9 * numpy.exp(0.7j), 0.9 * numpy.exp(-0.7j), 0.95, 0.5])
    P, Q = rng.randn(N, 2), rng.randn(N, 2)
    cols = []
    for t in range(K):
        z = lam[0]**t
        cols.append(30.0 * (z.real * P[:, 0] - z.imag * P[:, 1])
                    + 0.95**t * Q[:, 0] + 0.5**t * Q[:, 1])
    return numpy.array(cols).T, M, L, lam


def _gram(X, M):
    G = X.T.dot(M).dot(X)
    return 0.5 * (G + G.T)


def _report(what, err, bound):
    print('%s: error %.2e  bound %.2e' % (what, err, bound))
    assert err <= bound


# -- the host algebra against the SVD restatement -------------------------------------
def test_pod_from_gram_against_svd():
    '''Bound: 5 k eps lambda_1 / lambda_7 = 7.8e-9 (k = 7, lambda_1 /
    lambda_7 = 1e6).  Measured on the CPU, as fractions of k eps lambda_1 /
    lambda_7 = 1.55e-9: energies (relative to each) 0.027, M-orthonormality
    0.027, subspaces 0.0073, X = modes a 2.3e-7; the restatement's own Gram
    route against its SVD route, from which c = 5 is taken: 0.049, 0.049 and
    0.011.'''
    from flow_amd.fem.snapshots import pod_from_gram
    X, M, L = _pod_case()
    s, modes, coef = sref.pod_svd(X, L)
    assert numpy.abs(s - SIGMA).max() <= 1e-10 * SIGMA[0]
    bound = C_BOUND * K * EPS * (s[0] / s[-1])**2
    energies, C, a = pod_from_gram(_gram(X, M), None, 1e-10, False)
    assert energies.shape == (K,) and C.shape == (K, K) and a.shape == (K, K)
    _report('energies', numpy.abs((energies - s**2) / s**2).max(), bound)
    Phi = X.dot(C)
    _report('M-orthonormality',
            numpy.abs(Phi.T.dot(M).dot(Phi) - numpy.eye(K)).max(), bound)
    _report('subspaces', max(sref.subspace_gap(modes[:, g], Phi[:, g], M)
                             for g in GROUPS), bound)
    # the temporal coefficients reconstruct the snapshots
    _report('X = modes a', numpy.abs(Phi.dot(a) - X).max() / numpy.abs(X).max(),
            bound)


def test_dmd_from_gram_against_svd():
    '''Bound: 5 k eps sigma_1^2 / sigma_4^2 = 6.9e-10 (k = 7, the fourth
    singular value of X[:, :-1] being the smallest kept).  Measured on the
    CPU: eigenvalues against the restatement and against the map 3.2e-12
    (0.023 of k eps sigma_1^2 / sigma_4^2 = 1.39e-10; the restatement's own
    Gram route against its SVD route: 0.022), mode directions 0 to rounding,
    x_0 = modes b 7.1e-14.'''
    from flow_amd.fem.snapshots import dmd_from_gram
    X, M, L, lam_true = _dmd_case()
    s = numpy.linalg.svd(L.T.dot(X[:, :-1]), compute_uv=False)
    bound = C_BOUND * K * EPS * (s[0] / s[3])**2
    want, ref_modes = sref.dmd_svd(X, L, 4)
    lam, T, b, s2 = dmd_from_gram(_gram(X, M), 4, 1e-14)
    assert lam.shape == (4,) and T.shape == (K - 1, 4) and b.shape == (4,)
    assert s2.shape == (K - 1,)
    p = sref.match(lam, want)
    assert sorted(p.tolist()) == [0, 1, 2, 3]
    _report('eigenvalues against the restatement',
            numpy.abs(lam[p] - want).max(), bound)
    q = sref.match(lam, lam_true)
    _report('eigenvalues against the map', numpy.abs(lam[q] - lam_true).max(),
            bound)
    # the exact modes are eigenvectors of the map: parallel to the
    # restatement's, whatever the scaling of W
    Phi = X[:, 1:].dot(T)
    cosines = [abs(numpy.vdot(Phi[:, i], ref_modes[:, j]))
               / numpy.linalg.norm(Phi[:, i]) / numpy.linalg.norm(ref_modes[:, j])
               for j, i in enumerate(p)]
    _report('1 - |cos(mode, restatement)|', 1.0 - min(cosines), bound)
    # the amplitudes expand the first snapshot in the projected modes, which
    # for states inside the invariant subspace are the exact ones
    x0 = Phi.dot(b)
    assert numpy.abs(x0.imag).max() <= 1e-6 * numpy.abs(X[:, 0]).max()
    _report('x_0 = modes b', numpy.abs(x0.real - X[:, 0]).max()
            / numpy.abs(X[:, 0]).max(), bound)


def test_rank_truncation():
    from flow_amd.fem.snapshots import dmd_from_gram, pod_from_gram
    # lambda = 1, 1e-4, 1e-14 (sigma = 1, 1e-2, 1e-7): rtol acts on lambda
    G = numpy.diag([1.0, 1e-4, 1e-14])
    for rtol, r, want in ((1e-10, None, 2), (1e-16, None, 3), (1e-3, None, 1),
                          (1e-10, 1, 1), (1e-16, 5, 3)):
        energies, C, a = pod_from_gram(G, r, rtol, False)
        assert energies.shape == (3,)          # all of them, kept or not
        assert C.shape == (3, want) and a.shape == (want, 3)
    # a rank-one sequence x_t = 0.5^t x: one eigenvalue however many are asked
    g = 0.5**numpy.arange(5)
    lam, T, b, s2 = dmd_from_gram(numpy.outer(g, g), None, 1e-10)
    assert lam.shape == (1,) and abs(lam[0] - 0.5) <= 1e-14
    assert abs(b[0] * T[:, 0].dot(g[1:]) - 1.0) <= 1e-13
    for bad in (0, -1):
        with pytest.raises(ValueError, match='r:'):
            pod_from_gram(G, bad)
        with pytest.raises(ValueError, match='r:'):
            dmd_from_gram(G, bad)
    with pytest.raises(ValueError):
        dmd_from_gram(numpy.ones((1, 1)))
    with pytest.raises(ValueError, match='vanish'):
        dmd_from_gram(numpy.zeros((3, 3)))


def test_centring():
    '''Bound: 5 k eps lambda_1 / lambda_6 = 2.3e-9 of the centred snapshots
    (six modes: centring costs one rank).  Measured on the CPU: column sums
    of C 6.1e-17, energies 3.8e-11, M-orthonormality 3.8e-11, X - mean =
    modes a 3.5e-15, against the POD of X - mean 5.8e-11.'''
    from flow_amd.fem.snapshots import pod_from_gram
    X, M, L = _pod_case()
    X = X + 50.0 * numpy.linalg.solve(L.T, numpy.ones((N, 1)))     # a mean
    Xc = sref.centre(X)
    s, modes, coef = sref.pod_svd(Xc, L)
    keep = K - 1                                  # centring costs one rank
    bound = C_BOUND * K * EPS * (s[0] / s[keep - 1])**2
    energies, C, a = pod_from_gram(_gram(X, M), None, 1e-10, True)
    assert C.shape == (K, keep) and a.shape == (keep, K)
    _report('column sums of C', numpy.abs(C.sum(axis=0)).max()
            / numpy.abs(C).max(), bound)
    _report('energies', numpy.abs((energies[:keep] - s[:keep]**2)
                                  / s[:keep]**2).max(), bound)
    Phi = X.dot(C)
    _report('M-orthonormality',
            numpy.abs(Phi.T.dot(M).dot(Phi) - numpy.eye(keep)).max(), bound)
    _report('X - mean = modes a', numpy.abs(Phi.dot(a) - Xc).max()
            / numpy.abs(Xc).max(), bound)
    # the same as the uncentred POD of the centred snapshots
    e2, C2, a2 = pod_from_gram(_gram(Xc, M), None, 1e-10, False)
    _report('against the POD of X - mean', numpy.abs(
        (energies[:keep] - e2[:keep]) / e2[:keep]).max(), bound)


# -- the time step ----------------------------------------------------------------------
def test_dt_rules():
    from flow_amd.fem.snapshots import DMD, resolve_dt
    assert resolve_dt(0.25, []) == 0.25
    assert resolve_dt(0.25, [0.0, 1.0, 5.0]) == 0.25          # dt wins
    assert resolve_dt(None, [None, None, None]) is None
    assert resolve_dt(None, [0.0, None, 0.2]) is None
    assert resolve_dt(None, []) is None
    assert abs(resolve_dt(None, [0.1 * i for i in range(12)]) - 0.1) <= 1e-15
    with pytest.raises(ValueError, match='uniform'):
        resolve_dt(None, [0.0, 0.1, 0.3])
    with pytest.raises(ValueError, match='uniform'):
        resolve_dt(None, [0.0, 0.1, 0.1])
    with pytest.raises(ValueError, match='dt'):
        resolve_dt(0.0, [])
    lam = numpy.array([numpy.exp((-0.3 + 2.0j) * 0.1),
                       numpy.exp((-0.3 - 2.0j) * 0.1), numpy.exp(-0.5 * 0.1)])
    d = DMD(lam, numpy.ones(3), [], 0.1)
    assert d.r == 3 and d.eigenvalues.dtype == complex
    assert numpy.abs(d.frequencies - numpy.array([1.0, -1.0, 0.0]) / numpy.pi
                     ).max() <= 1e-14
    assert numpy.abs(d.growth_rates - [-0.3, -0.3, -0.5]).max() <= 1e-14
    d = DMD(lam, numpy.ones(3), [], None)
    for name in ('frequencies', 'growth_rates'):
        with pytest.raises(ValueError, match='time step'):
            getattr(d, name)


# -- refusals, the store's bookkeeping, exports, symbols ----------------------------------
def test_refusals(monkeypatch):
    mesh = fem.UnitSquareMesh(4, 4)
    other = fem.UnitSquareMesh(4, 4)
    P1, P2 = fem.FunctionSpace(mesh, 'CG', 1), fem.FunctionSpace(mesh, 'CG', 2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    mixed = fem.FunctionSpace(
        mesh, fem.VectorElement('CG', 'triangle', 2)
        * fem.FiniteElement('CG', 'triangle', 1))
    for V in (mixed, W.sub(0), W.sub(1)):
        with pytest.raises(NotImplementedError):
            fem.Snapshots(V, 4)

    class Cubic(object):
        layout, component, degree, dim = P2.layout, None, 3, 1

    class Triple(object):
        layout, component, degree, dim = P2.layout, None, 2, 3

    with pytest.raises(ValueError, match='P3'):
        fem.Snapshots(Cubic(), 4)
    with pytest.raises(ValueError, match='3 components'):
        fem.Snapshots(Triple(), 4)
    with pytest.raises(ValueError, match='lumped'):
        fem.Snapshots(P2, 4, inner='lumped')
    with pytest.raises(ValueError, match='lumped'):
        fem.Snapshots(W, 4, inner='lumped')
    with pytest.raises(ValueError, match='inner'):
        fem.Snapshots(P1, 4, inner='H1')
    with pytest.raises(ValueError, match='capacity'):
        fem.Snapshots(P1, 0)
    S = fem.Snapshots(P2, 4)
    assert len(S) == 0 and S.times == [] and S.capacity == 4
    assert S.n == P2.N and S.ld == P2.N + (P2.N & 1)
    SW = fem.Snapshots(W, 3, inner='l2')
    assert SW.n == 2 * W.N and SW.ld % 2 == 0 and SW.ld - SW.n in (0, 1)
    assert SW._X.numel() == 3 * SW.ld
    for bad in (fem.Function(P1), fem.Function(W),
                fem.Function(fem.FunctionSpace(other, 'CG', 2)), 3.0,
                fem.Constant(1.0)):
        with pytest.raises(ValueError, match='u:'):
            S.append(bad)
    assert len(S) == 0
    for call in (S.mean, S.pod):
        with pytest.raises(ValueError, match='no snapshots'):
            call()
    with pytest.raises(ValueError, match='two snapshots'):
        S.dmd()
    with pytest.raises(IndexError):
        S.column(0)
    from flow_amd import parallel
    monkeypatch.setattr(parallel, 'active', lambda: True)
    for call in (lambda: fem.Snapshots(P2, 4),
                 lambda: S.append(fem.Function(P2))):
        with pytest.raises(NotImplementedError, match='on strips'):
            call()


def test_capacity_overflow_and_bookkeeping(monkeypatch):
    '''The store's host side, with the device part of append (the Gram row)
    replaced by writing known numbers: columns are copied in order, the
    append past `capacity` is refused and leaves the store as it was, gram()
    mirrors the lower triangle, clear() empties.'''
    import torch
    from flow_amd.fem.snapshots import Snapshots
    V = fem.FunctionSpace(fem.UnitSquareMesh(2, 2), 'CG', 1)          # N = 9
    S = Snapshots(V, 3, inner='l2')
    assert S.ld == 10

    def row(k):
        S._G[k * S.capacity:k * S.capacity + k + 1] = torch.arange(
            1.0, k + 2.0, dtype=torch.float64) + 10.0 * k
    monkeypatch.setattr(S, '_gram_row', row)
    fs = []
    for k in range(3):
        u = fem.Function(V)
        u.set_array(numpy.arange(9.0) + 100.0 * k)
        S.append(u, t=0.5 * k)
        fs.append(u)
    assert len(S) == 3 and S.times == [0.0, 0.5, 1.0]
    with pytest.raises(ValueError, match='full'):
        S.append(fs[0], t=1.5)
    assert len(S) == 3 and S.times == [0.0, 0.5, 1.0]
    for k in range(3):
        assert numpy.array_equal(S.column(k).array(), fs[k].array())
    out = fem.Function(V)
    assert S.column(1, out=out) is out
    assert numpy.array_equal(out.array(), fs[1].array())
    G = S.gram()
    assert G.shape == (3, 3) and numpy.array_equal(G, G.T)
    assert numpy.array_equal(G, [[1.0, 11.0, 21.0], [11.0, 12.0, 22.0],
                                 [21.0, 22.0, 23.0]])
    S.clear()
    assert len(S) == 0 and S.times == []
    S.append(fs[2])
    assert S.times == [None] and S.gram().shape == (1, 1)
    assert numpy.array_equal(S.column(0).array(), fs[2].array())


def test_exports():
    from flow_amd.fem import snapshots
    assert fem.Snapshots is snapshots.Snapshots
    for name in ('pod_from_gram', 'dmd_from_gram', 'POD', 'DMD'):
        assert hasattr(snapshots, name)


def test_symbols_declared_and_bound():
    from flow_amd import _hip
    with open(os.path.join(ROOT, 'include', 'flow_hip.h')) as f:
        header = f.read()
    lib = _hip.load_library()
    assert lib.flow_abi_version() == _hip.ABI_VERSION
    for name, nargs in (('flow_multi_dot', 8), ('flow_combine', 10)):
        assert 'int %s(' % name in header
        assert len(_hip.SYMBOLS[name]) == nargs
        decl = header[header.index('int %s(' % name):]
        assert decl[:decl.index(';')].count(',') == nargs - 1
        assert getattr(lib, name) is not None
    assert '#define FLOW_MULTI_DOT_BLOCKS %d' % _hip.MULTI_DOT_BLOCKS in header
    # size_t strides: a store of more than 2^31 doubles is addressed
    import ctypes
    assert _hip.SYMBOLS['flow_multi_dot'][3] is ctypes.c_size_t
    assert _hip.SYMBOLS['flow_combine'][3] is ctypes.c_size_t
    assert _hip.SYMBOLS['flow_combine'][8] is ctypes.c_size_t
    # argument checks that need no device: nothing to do, and bad strides
    assert lib.flow_multi_dot(0, 3, None, 0, None, None, None, None) == 0
    assert lib.flow_multi_dot(5, 0, None, 6, None, None, None, None) == 0
    assert lib.flow_combine(0, 1, None, 0, 1, None, None, None, 0, None) == 0
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.flow_multi_dot(5, 1, p, 5, p, p, p, None) == 2       # odd ldx
    assert lib.flow_multi_dot(5, 1, p, 4, p, p, p, None) == 2       # ldx < n
    assert b'ldx' in lib.flow_last_error()
    assert lib.flow_combine(5, 1, p, 6, 1, p, None, p, 6, None) == 2
    assert b'overlap' in lib.flow_last_error()
