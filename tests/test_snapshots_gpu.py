# -*- coding: utf-8 -*-
'''
fem.Snapshots on the HIP path (flow_amd/fem/snapshots.py; csrc/
snapshot_kernels.hip): the two kernels against numpy, the store end to end
against the restatement of tests/snapshots_reference.py, and a sequence whose
decomposition is known in closed form.

Bounds (every test prints its measured error next to its bound, pytest -s):

flow_multi_dot   n eps sum_i |x_i| |y_i| per entry: n fma roundings of partial
                 sums that never exceed sum |x||y|, whatever the order.
flow_combine     m eps sum_j |C_kj| |X_ji| per entry, against a long double
                 reference.  The chain starts from base[i], so its partial
                 sums stay below |base_i| + sum |C||X| and its m roundings
                 below m eps/2 (|base_i| + sum |C||X|): within the bound as
                 long as |base_i| <= sum |C||X|, and the base of this test is
                 half the smallest such sum.
Snapshots        a Gram entry: (n + 32) eps (|X|^T |W| |X|)_ij, the multi-dot
                 bound with the rounding of y = W x (rows of at most 32
                 entries) in front.  Everything that goes through the
                 eigenvectors of G: (5 k + n) eps lambda_1 / lambda_r -- the
                 rounding of G, n eps lambda_1, seen by the smallest kept
                 eigenvalue, on top of the host algebra's 5 k eps lambda_1 /
                 lambda_r (tests/test_snapshots_host.py, where the 5 comes
                 from); lambda from the restatement's SVD.

                 The mean: (k + 1) eps mean_j |x_ji| -- k fma roundings of
                 the kernel, as many of numpy's, and the rounding of 1 / k.

Sizes: n = 1, 255, 257 (one row; less and more than one block of rows), 4099
(odd, several blocks), kRedBlocks * kBlock + 1 (the multi-dot grid at its
1024 blocks, the combine grid one block past them) and 2 * kRedBlocks *
kBlock + 5, where a multi-dot lane, which takes its entries in pairs, runs
its grid stride a second time and the odd last entry falls to a lane in its
second turn.  The padding of every column is NaN: a read past n shows.
'''
import ctypes
import functools

import numpy
import pytest
import torch

from flow_amd import _hip, device, fem
from flow_amd.fem import Snapshots

import recovery_reference as rref
import snapshots_reference as sref

pytestmark = pytest.mark.gpu

EPS = numpy.finfo(float).eps
KRED, KBLOCK = 1024, 256
SIZES = [1, 255, 257, 4099, KRED * KBLOCK + 1, 2 * KRED * KBLOCK + 5]
MMAX = 17
C_HOST = 5.0          # tests/test_snapshots_host.py


def _report(what, err, bound):
    print('%s: error %.2e  bound %.2e' % (what, err, bound))
    assert numpy.isfinite(err) and err <= bound


def _ld(n):
    return (n + 3) & ~1          # even and > n


@functools.lru_cache(maxsize=2)
def _columns(n):
    '''(X host (MMAX, ld) with NaN padding, y host, X device, y device).'''
    rng = numpy.random.RandomState(n % 1000 + 1)
    ld = _ld(n)
    X = numpy.full((MMAX, ld), numpy.nan)
    X[:, :n] = rng.uniform(-1.0, 1.0, size=(MMAX, n))
    y = rng.uniform(-1.0, 1.0, size=n)
    X.flags.writeable = False
    y.flags.writeable = False
    return X, y, device.to_device(X.reshape(-1)), device.to_device(y)


def _multi_dot(lib, n, m, Xd, ld, yd, first=0):
    out = device.empty(m)
    out.fill_(float('nan'))
    work = device.empty(m * KRED)
    _hip.check(lib.flow_multi_dot(
        n, m, _hip.f64(Xd[first * ld:], (m - 1) * ld + n), ld, _hip.f64(yd, n),
        _hip.f64(work), _hip.f64(out, m), _hip.stream()))
    return device.to_host(out).numpy()


def _combine(lib, n, m, Xd, ld, Cd, r, based, ldo):
    out = device.empty(r * ldo)
    out.fill_(-7.0)
    _hip.check(lib.flow_combine(
        n, m, _hip.f64(Xd, (m - 1) * ld + n), ld, r, _hip.f64(Cd, r * m),
        None if based is None else _hip.f64(based, n),
        _hip.f64(out, (r - 1) * ldo + n), ldo, _hip.stream()))
    return device.to_host(out).numpy().reshape(r, ldo)


# -- 1. flow_multi_dot -------------------------------------------------------------------
@pytest.mark.parametrize('m', [1, 7, 8, 9, 17])
@pytest.mark.parametrize('n', SIZES)
def test_multi_dot_against_numpy(hip, n, m):
    X, y, Xd, yd = _columns(n)
    got = _multi_dot(hip, n, m, Xd, _ld(n), yd)
    want = X[:m, :n].dot(y)
    bound = n * EPS * numpy.abs(X[:m, :n]).dot(numpy.abs(y))
    ratio = (numpy.abs(got - want) / bound).max()
    print('n %d m %d: largest error / bound %.2e (bound %.2e .. %.2e)'
          % (n, m, ratio, bound.min(), bound.max()))
    assert numpy.isfinite(got).all() and ratio <= 1.0
    again = _multi_dot(hip, n, m, Xd, _ld(n), yd)
    assert numpy.array_equal(got.view(numpy.int64), again.view(numpy.int64))


@pytest.mark.parametrize('n', [257, 4099, SIZES[-1]])
def test_multi_dot_entry_depends_on_its_column_alone(hip, n):
    '''Entry j of the m = 17 call (chunks 0-7 and 8-15, then column 16 alone)
    has the bits of the m = 1 call on column j, for every j, that is for
    every position in a chunk, and the bits of entry j of the m = 7, 8 and 9
    calls (other chunk sizes, other chunk positions).'''
    X, y, Xd, yd = _columns(n)
    ld = _ld(n)
    full = _multi_dot(hip, n, MMAX, Xd, ld, yd).view(numpy.int64)
    for j in range(MMAX):
        one = _multi_dot(hip, n, 1, Xd, ld, yd, first=j).view(numpy.int64)
        assert one[0] == full[j], j
    for m in (7, 8, 9):
        part = _multi_dot(hip, n, m, Xd, ld, yd).view(numpy.int64)
        assert numpy.array_equal(part, full[:m]), m
        # ... and starting at another column: position j - 3 in its chunk
        part = _multi_dot(hip, n, m, Xd, ld, yd, first=3).view(numpy.int64)
        assert numpy.array_equal(part, full[3:3 + m]), m


def test_multi_dot_nothing_to_do_and_refusals(hip):
    X, y, Xd, yd = _columns(255)
    out = device.empty(4)
    out.fill_(3.0)
    work = device.empty(4 * KRED)
    args = (_hip.f64(Xd), 256, _hip.f64(yd), _hip.f64(work), _hip.f64(out),
            _hip.stream())
    before = _hip.launch_count()
    assert hip.flow_multi_dot(0, 4, *args) == 0
    assert hip.flow_multi_dot(255, 0, *args) == 0
    assert _hip.launch_count() == before
    assert device.to_host(out).numpy().tolist() == [3.0] * 4
    with pytest.raises(ValueError, match='ldx'):
        _hip.check(hip.flow_multi_dot(255, 1, _hip.f64(Xd), 257, *args[2:]))
    with pytest.raises(ValueError, match='aligned'):
        _hip.check(hip.flow_multi_dot(
            200, 1, ctypes.c_void_p(Xd.data_ptr() + 8), 256, *args[2:]))


# -- 2. flow_combine ---------------------------------------------------------------------
@pytest.mark.parametrize('with_base', [False, True])
@pytest.mark.parametrize('r', [1, 8, 9])
@pytest.mark.parametrize('m', [1, 9])
@pytest.mark.parametrize('n', SIZES)
def test_combine_against_numpy(hip, n, m, r, with_base):
    X, y, Xd, yd = _columns(n)
    ld, ldo = _ld(n), n + 5
    rng = numpy.random.RandomState(100 * m + r)
    C = rng.uniform(-1.0, 1.0, size=(r, m))
    S = numpy.abs(C).dot(numpy.abs(X[:m, :n]))                     # (r, n)
    base = based = None
    if with_base:
        base = 0.5 * S.min() * rng.uniform(-1.0, 1.0, size=n)
        based = device.to_device(base)
    Cd = device.to_device(C.reshape(-1))
    got = _combine(hip, n, m, Xd, ld, Cd, r, based, ldo)
    assert (got[:, n:] == -7.0).all()          # the padding is not written
    want = C.astype(numpy.longdouble).dot(X[:m, :n].astype(numpy.longdouble))
    if with_base:
        want = want + base
    bound = m * EPS * S
    err = numpy.abs(got[:, :n] - want).astype(float)
    ok = bound > 0.0
    ratio = (err[ok] / bound[ok]).max() if ok.any() else 0.0
    print('n %d m %d r %d base %d: largest error / bound %.2e (bound up to '
          '%.2e)' % (n, m, r, with_base, ratio, bound.max()))
    assert numpy.isfinite(got[:, :n]).all()
    assert ratio <= 1.0 and (err[~ok] == 0.0).all()
    again = _combine(hip, n, m, Xd, ld, Cd, r, based, ldo)
    assert numpy.array_equal(got[:, :n].view(numpy.int64),
                             again[:, :n].view(numpy.int64))


def test_combine_long_sum_and_refusals(hip):
    '''m = 17 columns (no multiple of the staged tile is needed for one tile;
    the store of the end-to-end tests below never holds more than a few) and
    m = 70 over a store that repeats the 17 columns: three staged tiles of
    32, the last one ragged.'''
    n = 4099
    X, y, Xd, yd = _columns(n)
    ld = _ld(n)
    reps = 5
    big = device.to_device(numpy.tile(X.reshape(-1), reps))
    Xh = numpy.tile(X, (reps, 1))
    for m, r in ((17, 3), (70, 9)):
        C = numpy.random.RandomState(m).uniform(-1.0, 1.0, size=(r, m))
        Cd = device.to_device(C.reshape(-1))
        got = _combine(hip, n, m, big, ld, Cd, r, None, ld)[:, :n]
        want = C.astype(numpy.longdouble).dot(
            Xh[:m, :n].astype(numpy.longdouble))
        bound = m * EPS * numpy.abs(C).dot(numpy.abs(Xh[:m, :n]))
        _report('m %d r %d: largest error / bound' % (m, r),
                (numpy.abs(got - want).astype(float) / bound).max(), 1.0)
    out = device.empty(2 * ld)
    with pytest.raises(ValueError, match='overlaps X'):
        _hip.check(hip.flow_combine(
            n, 2, _hip.f64(Xd), ld, 1, _hip.f64(Cd), None,
            _hip.f64(Xd[ld:]), ld, _hip.stream()))
    with pytest.raises(ValueError, match='overlaps base'):
        _hip.check(hip.flow_combine(
            n, 2, _hip.f64(Xd), ld, 2, _hip.f64(Cd), _hip.f64(out[ld:]),
            _hip.f64(out), ld, _hip.stream()))


# -- 3. Snapshots end to end -------------------------------------------------------------
FIELDS = [
    (lambda x, y: numpy.sin(3 * x + 1) * numpy.exp(y),
     lambda x, y: numpy.cos(2 * y - x)),
    (lambda x, y: numpy.cos(4 * y - x),
     lambda x, y: x * x - y),
    (lambda x, y: 1 + x * y,
     lambda x, y: numpy.sin(5 * x) * numpy.sin(4 * y)),
    (lambda x, y: numpy.sin(5 * x) * numpy.sin(4 * y) + 0.3,
     lambda x, y: numpy.exp(-x) * numpy.cos(2 * y)),
    (lambda x, y: numpy.exp(-x) * numpy.cos(2 * y) + y * y,
     lambda x, y: 2 - x + numpy.sin(3 * y)),
]
K = len(FIELDS)
CASES = [(name, deg, dim, inner)
         for name in rref.MESHES for deg in (1, 2) for dim in (1, 2)
         for inner in ('L2', 'lumped', 'l2') if inner != 'lumped' or deg == 1]


@functools.lru_cache(maxsize=None)
def _weight(name, deg, inner):
    V = fem.FunctionSpace(rref.mesh(name), 'CG', deg)
    W = sref.weight_matrix(V, inner)
    W.flags.writeable = False
    return W


@functools.lru_cache(maxsize=None)
def _fields(name, deg, dim):
    V = fem.FunctionSpace(rref.mesh(name), 'CG', deg, dim=dim)
    us = [rref.field(V, list(f[:dim])) for f in FIELDS]
    X = numpy.array([u.array() for u in us]).T                     # (n, K)
    X.flags.writeable = False
    return V, us, X


@pytest.mark.parametrize('name,deg,dim,inner', CASES)
def test_snapshots_against_reference(hip, name, deg, dim, inner):
    V, us, X = _fields(name, deg, dim)
    W = _weight(name, deg, inner)
    n = X.shape[0]
    tag = '%s P%d x%d %s' % (name, deg, dim, inner)
    S = Snapshots(V, K + 1, inner=inner)
    for j, u in enumerate(us):
        S.append(u, t=0.1 * j)
    assert len(S) == K and S.times == [0.1 * j for j in range(K)]
    for j in (0, K - 1):
        assert numpy.array_equal(S.column(j).array(), X[:, j])
    # the Gram matrix
    G = S.gram()
    assert G.shape == (K, K) and numpy.array_equal(G, G.T)
    Gref = sref.gram(V, W, X)
    Gbound = (n + 32) * EPS * sref.gram(V, numpy.abs(W), numpy.abs(X))
    _report(tag + ' gram, largest error / bound',
            (numpy.abs(G - Gref) / Gbound).max(), 1.0)
    # the mean
    mean = S.mean()
    assert isinstance(mean, fem.Function) and mean.function_space().same_as(V)
    _report(tag + ' mean, largest error / bound',
            (numpy.abs(mean.array() - X.mean(axis=1))
             / ((K + 1) * EPS * numpy.abs(X).mean(axis=1) + 1e-300)).max(), 1.0)
    # POD about the mean: K - 1 modes, orthonormal, and they give the
    # snapshots back
    Xc = sref.centre(X)
    lam = numpy.linalg.eigvalsh(sref.gram(V, W, Xc))[::-1]
    bound = (C_HOST * K + n) * EPS * lam[0] / lam[K - 2]
    assert bound < 1e-6, (tag, lam)
    pod = S.pod()
    assert pod.r == K - 1 == len(pod.modes) and pod.energies.shape == (K,)
    assert pod.coefficients.shape == (K - 1, K)
    _report(tag + ' energies', numpy.abs(
        (pod.energies[:K - 1] - lam[:K - 1]) / lam[:K - 1]).max(), bound)
    Phi = numpy.array([f.array() for f in pod.modes]).T
    _report(tag + ' orthonormality', numpy.abs(
        Phi.T.dot(sref.weighted(V, W, Phi)) - numpy.eye(K - 1)).max(), bound)
    assert numpy.array_equal(pod.mean.array(), mean.array())
    scale = numpy.abs(X).max()
    out = fem.Function(V)
    worst = 0.0
    for j in range(K):
        back = pod.reconstruct(pod.coefficients[:, j], out=out)
        assert back is out
        worst = max(worst, numpy.abs(back.array() - X[:, j]).max() / scale)
    _report(tag + ' reconstruction', worst, bound)
    a = numpy.sqrt(lam[0]) * numpy.array([1.0, -0.5, 0.25, 2.0][:K - 1])
    got = pod.project(pod.reconstruct(a))
    assert isinstance(got, numpy.ndarray) and got.shape == (K - 1,)
    _report(tag + ' project(reconstruct(a))',
            numpy.abs(got - a).max() / numpy.abs(a).max(), bound)
    # a Gram row written at append time is the row a later batch computes
    y = S._weight.apply(S._col(K - 1), S._y[:n])
    row = _multi_dot(hip, n, K, S._X, S.ld, y)
    assert S._work.numel() == S.capacity * KRED
    assert numpy.array_equal(row.view(numpy.int64),
                             G[K - 1].view(numpy.int64))


def test_snapshots_store_rules(hip):
    V, us, X = _fields('square 2', 1, 2)           # N = 9: an odd ld - 1
    S = Snapshots(V, 2, inner='L2')
    assert S.n == 18 and S.ld == 18
    V1, us1, X1 = _fields('square 2', 1, 1)
    S1 = Snapshots(V1, 2, inner='L2')
    assert S1.n == 9 and S1.ld == 10
    S.append(us[0])
    S.append(us[1])
    with pytest.raises(ValueError, match='full'):
        S.append(us[2])
    assert len(S) == 2 and S.times == [None, None]
    G = S.gram()
    S.clear()
    assert len(S) == 0
    S.append(us[1])
    S.append(us[0])
    G2 = S.gram()
    # the same pairs of columns, appended in the other order: the same bits
    assert G2[0, 0] == G[1, 1] and G2[1, 1] == G[0, 0]
    d = S.dmd()
    assert d.r >= 1 and d.dt is None
    with pytest.raises(ValueError, match='time step'):
        d.frequencies
    # without the mean: every snapshot counts
    pod = S.pod(subtract_mean=False)
    assert pod.mean is None and pod.r == 2


# -- 4. a sequence with a known decomposition -----------------------------------------------
WAVE, DT, NT = 2 * numpy.pi, 0.1, 12
OMEGA = 2 * numpy.pi / (NT * DT)            # one period in the 12 snapshots
DECAY = 0.8


def _sequence(with_decay):
    '''Interpolants on P2 over UnitSquareMesh(12, 12) of sin(k x - omega t)
    [+ exp(-decay t) g(x, y)] at t = 0, dt, ...: rank 2 [3] exactly (the time
    dependence factors out of the interpolation), linear dynamics with the
    eigenvalues exp(+-i omega dt) [and exp(-decay dt)].'''
    V = fem.FunctionSpace(fem.UnitSquareMesh(12, 12), 'CG', 2)
    us = []
    for j in range(NT):
        t = j * DT
        us.append(rref.field(V, [lambda x, y: numpy.sin(WAVE * x - OMEGA * t)
                                 + (numpy.exp(-DECAY * t) * numpy.cos(3 * y)
                                    * (1 + x) if with_decay else 0.0)]))
    return V, us, numpy.array([u.array() for u in us]).T


def test_dmd_of_a_travelling_and_a_decaying_wave(hip):
    V, us, X = _sequence(True)
    n = X.shape[0]
    M = sref.mass_matrix(V)
    L = numpy.linalg.cholesky(M)
    s = numpy.linalg.svd(L.T.dot(X[:, :-1]), compute_uv=False)
    assert s[3] <= 1e-12 * s[0]                    # rank 3
    want = numpy.array([numpy.exp(1j * OMEGA * DT), numpy.exp(-1j * OMEGA * DT),
                        numpy.exp(-DECAY * DT)])
    ref, _ = sref.dmd_svd(X, L, 3)
    print('restatement against the closed form: %.2e'
          % numpy.abs(ref[sref.match(ref, want)] - want).max())
    bound = (C_HOST * NT + n) * EPS * (s[0] / s[2])**2
    assert bound < 1e-8
    S = Snapshots(V, NT, inner='L2')
    for j, u in enumerate(us):
        S.append(u, t=j * DT)
    d = S.dmd(r=3)
    assert d.r == 3 and len(d.modes) == 3 and abs(d.dt - DT) <= 1e-15
    p = sref.match(d.eigenvalues, want)
    assert sorted(p.tolist()) == [0, 1, 2]
    _report('eigenvalues', numpy.abs(d.eigenvalues[p] - want).max(), bound)
    _report('frequencies', numpy.abs(
        d.frequencies[p] - numpy.array([1.0, -1.0, 0.0]) * OMEGA
        / (2 * numpy.pi)).max(), bound / (2 * numpy.pi * DT * numpy.abs(want).min()))
    _report('growth rates', numpy.abs(
        d.growth_rates[p] - [0.0, 0.0, -DECAY]).max(),
        bound / (DT * numpy.abs(want).min()))
    # the modes are Functions of V; that of the decaying eigenvalue is real
    # and parallel to the interpolant of g
    re, im = d.modes[p[2]]
    assert isinstance(re, fem.Function) and re.function_space().same_as(V)
    xy = V.layout.dof_coords
    g = numpy.cos(3 * xy[:, 1]) * (1 + xy[:, 0])
    ra = re.array()
    cosine = abs(ra.dot(g)) / numpy.linalg.norm(ra) / numpy.linalg.norm(g)
    _report('1 - |cos(decaying mode, g)|', 1.0 - cosine, bound)
    assert numpy.abs(im.array()).max() <= bound * numpy.abs(ra).max()
    # a time step handed in wins over the times
    assert S.dmd(r=3, dt=0.2).dt == 0.2


def test_pod_of_a_travelling_wave_has_two_equal_energies(hip):
    V, us, X = _sequence(False)
    n = X.shape[0]
    L = numpy.linalg.cholesky(sref.mass_matrix(V))
    s, _, _ = sref.pod_svd(X, L)
    print('restatement: sigma^2 = %.15e, %.15e, then %.2e'
          % (s[0]**2, s[1]**2, s[2]**2))
    bound = (C_HOST * NT + n) * EPS
    assert abs(s[0]**2 - s[1]**2) <= bound * s[0]**2 and s[2] <= 1e-12 * s[0]
    S = Snapshots(V, NT, inner='L2')
    for u in us:
        S.append(u)
    pod = S.pod(subtract_mean=False)
    e = pod.energies
    assert pod.r == 2
    _report('energies against the restatement',
            numpy.abs(e[:2] - s[:2]**2).max() / s[0]**2, bound)
    _report('(lambda_1 - lambda_2) / lambda_1', (e[0] - e[1]) / e[0], bound)
    _report('lambda_3 / lambda_1', abs(e[2]) / e[0], bound)
