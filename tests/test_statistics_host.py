# -*- coding: utf-8 -*-
'''
fem.Statistics without a GPU (flow_amd/fem/statistics.py): every refusal
(raised before the device is touched), the store's layout, the symbols and
their argument checks on the loaded library, and the float64 restatement of
tests/statistics_reference.py against its own long-double two-pass reference
within the bounds the GPU tests use -- the bounds are checked here, on the
CPU, before any GPU run.

The bound.  Per entry, error <= C k eps scale with C = 5, k >= 10 samples
and f |t| <= k, the scales being max_j |x_ji| (mean), sum_j w_j (|x_ji| +
max_j |x_ji|)^2 (M2) and sum_j w_j |x_ji| (Fourier sums); extrema and their
times exact.  C is derived in the docstring of tests/test_statistics_gpu.py by
counting roundings, with one more per fma for the unfused restatement (p = 1
there): mean (3 k + 4) eps / 2, M2 (9 k + 5) eps / 2, Fourier sums (2 k +
2 pi f |t| + 15.6) eps / 2, merged halves (4.5 k + 9.5) eps, which is why the
merge below takes k = 20 samples.  Measured here (largest error / bound over
all entries; `pytest -s` prints them): 0.068 for the updates (a Fourier sum),
0.017 for the merged halves.
'''
import ctypes
import os

import numpy
import pytest

from flow_amd import fem
from flow_amd.fem import statistics

import statistics_reference as stref
from statistics_reference import EPS, Restatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 12
FREQS8 = (0.05, 0.11, 0.17, 0.23, 0.31, 0.4, 0.5, 0.6)     # f t <= 0.6 * 18 < K


def _bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.int64)


# -- refusals ---------------------------------------------------------------------------
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
            fem.Statistics(V)

    class Cubic(object):
        layout, component, degree, dim = P2.layout, None, 3, 1

    class Triple(object):
        layout, component, degree, dim = P2.layout, None, 2, 3

    with pytest.raises(ValueError, match='P3'):
        fem.Statistics(Cubic())
    with pytest.raises(ValueError, match='3 components'):
        fem.Statistics(Triple())
    with pytest.raises(ValueError, match='at most 8'):
        fem.Statistics(P1, frequencies=[0.1 * (i + 1) for i in range(9)])
    for bad in ((0.0,), (-1.0,), (1.0, float('nan')), (float('inf'),)):
        with pytest.raises(ValueError, match='frequencies'):
            fem.Statistics(P1, frequencies=bad)
    # update: all refused before the library is asked for a device
    S = fem.Statistics(P2)
    u = fem.Function(P2)
    for bad in (fem.Function(P1), fem.Function(W),
                fem.Function(fem.FunctionSpace(other, 'CG', 2)), 3.0,
                fem.Constant(1.0)):
        with pytest.raises(ValueError, match='u:'):
            S.update(bad)
    for bad in (0.0, -0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='dt'):
            S.update(u, dt=bad)
    for opts in (dict(frequencies=(1.0,)), dict(extrema=True)):
        St = fem.Statistics(P2, **opts)
        with pytest.raises(ValueError, match='t:'):
            St.update(u, dt=0.1)
        with pytest.raises(ValueError, match='t:'):
            St.update(u, dt=0.1, t=float('nan'))
    assert S.weight == 0.0 and S.count == 0 and S.t_first is None
    # empty statistics: every getter
    SW = fem.Statistics(W, frequencies=(1.0,), extrema=True)
    for call in (SW.mean, SW.variance, SW.rms, SW.covariance, SW.tke,
                 lambda: SW.fourier(0), SW.minimum, SW.maximum,
                 SW.time_of_minimum, SW.time_of_maximum):
        with pytest.raises(ValueError, match='no samples'):
            call()
    with pytest.raises(IndexError):
        SW.fourier(1)
    with pytest.raises(ValueError, match='2-vector'):
        S.tke()
    bare = fem.Statistics(P2, covariance=False)
    for call in (bare.variance, bare.rms, bare.covariance):
        with pytest.raises(ValueError, match='covariance=False'):
            call()
    with pytest.raises(ValueError, match='extrema=False'):
        bare.minimum()
    # merge: the same space, options and frequencies
    for wrong in (fem.Statistics(P1), fem.Statistics(W),
                  fem.Statistics(P2, covariance=False),
                  fem.Statistics(P2, extrema=True),
                  fem.Statistics(P2, frequencies=(1.0,)),
                  fem.Statistics(fem.FunctionSpace(other, 'CG', 2)), S, 3.0):
        with pytest.raises(ValueError, match='other'):
            S.merge(wrong)
    with pytest.raises(ValueError, match='other'):
        fem.Statistics(P2, frequencies=(1.0,)).merge(
            fem.Statistics(P2, frequencies=(2.0,)))
    # strips
    from flow_amd import parallel
    monkeypatch.setattr(parallel, 'active', lambda: True)
    for call in (lambda: fem.Statistics(P2), lambda: S.update(u),
                 lambda: S.merge(fem.Statistics.__new__(fem.Statistics))):
        with pytest.raises(NotImplementedError, match='on strips'):
            call()


def test_store_layout_and_state_refusals():
    assert fem.Statistics is statistics.Statistics
    assert statistics.MAX_FREQ == 8
    mesh = fem.UnitSquareMesh(2, 2)                       # P1: N = 9, odd
    P1 = fem.FunctionSpace(mesh, 'CG', 1)
    W = fem.VectorFunctionSpace(mesh, 'CG', 1)
    S = fem.Statistics(P1)
    assert (S.N, S.ld, S.planes) == (9, 10, 2)
    assert S._P.numel() == 20
    assert fem.Statistics(P1, covariance=False).planes == 1
    SW = fem.Statistics(W, frequencies=(0.5, 1.0), extrema=True)
    assert SW.planes == 2 + 3 + 2 * 2 * 2 + 4 * 2 and SW.ld == 10
    assert SW._at == {'mean': 0, 'M2': 2, 'fourier': 5, 'min': 13, 'max': 15,
                      'tmin': 17, 'tmax': 19}
    assert SW.scalar_space.dim == 1 and SW.scalar_space.degree == 1
    assert S.scalar_space is P1
    # the reset store, read back through state(): host tensors here
    st = SW.state()
    P = st['planes']
    assert P.shape == (21, 9) and (P[:13] == 0.0).all()
    assert (P[13:15] == numpy.inf).all() and (P[15:17] == -numpy.inf).all()
    assert numpy.isnan(P[17:]).all()
    assert st['weight'] == 0.0 and st['count'] == 0 and st['t_first'] is None
    # a round trip, and the mismatches
    st['weight'], st['count'], st['t_first'], st['t_last'] = 2.5, 3, 0.1, 0.7
    st['planes'][0] = numpy.arange(9.0)
    back = fem.Statistics.from_state(W, st)
    assert (back.weight, back.count, back.t_first, back.t_last) \
        == (2.5, 3, 0.1, 0.7)
    assert back.frequencies == (0.5, 1.0) and back.extrema
    assert numpy.array_equal(_bits(back.state()['planes']), _bits(st['planes']))
    with pytest.raises(ValueError, match='state'):
        fem.Statistics.from_state(P1, st)
    with pytest.raises(ValueError, match='state'):
        fem.Statistics.from_state(fem.VectorFunctionSpace(mesh, 'CG', 2), st)
    for key, bad in (('planes', st['planes'][:-1]), ('extrema', False),
                     ('frequencies', numpy.array([0.5])), ('weight', -1.0),
                     ('N', 8)):
        wrong = dict(st)
        wrong[key] = bad
        with pytest.raises(ValueError, match='state'):
            fem.Statistics.from_state(W, wrong)
    wrong = dict(st)
    del wrong['count']
    with pytest.raises(ValueError, match='state'):
        fem.Statistics.from_state(W, wrong)


def test_host_scalars_match_the_restatement():
    fourier_coefficients, merge_scalars, update_scalars = (
        statistics.fourier_coefficients, statistics.merge_scalars,
        statistics.update_scalars)
    assert update_scalars(0.0, 0.3) == (0.3, 1.0, 0.0)
    R = Restatement(1, 1, frequencies=(0.37,))
    R.update([1.0], 0.3, 0.0)
    R.update([2.0], 0.45, 1.7)
    W1, r, s = update_scalars(0.3, 0.45)
    assert W1 == R.W and R.mean[0, 0] == 1.0 + r * 1.0 and R.M2[0, 0] == s
    (c, sn), = fourier_coefficients((0.37,), 0.45, 1.7)
    assert R.A[0, 0, 0] == 0.3 * 1.0 + c * 2.0 and R.B[0, 0, 0] == sn * 2.0
    assert merge_scalars(1.0, 3.0) == (4.0, 0.75, 0.75)


# -- the symbols ------------------------------------------------------------------------
def test_symbols_declared_and_bound():
    from flow_amd import _hip
    with open(os.path.join(ROOT, 'include', 'flow_hip.h')) as f:
        header = f.read()
    lib = _hip.load_library()
    assert lib.flow_abi_version() == _hip.ABI_VERSION == 30
    for name, nargs in (('flow_stats_update', 11), ('flow_stats_merge', 10)):
        assert 'int %s(' % name in header
        assert len(_hip.SYMBOLS[name]) == nargs
        decl = header[header.index('int %s(' % name):]
        assert decl[:decl.index(';')].count(',') == nargs - 1
        assert getattr(lib, name) is not None
    assert '#define FLOW_STATS_MAX_FREQ %d' % _hip.STATS_MAX_FREQ in header
    assert '#define FLOW_STATS_COVARIANCE %d' % _hip.STATS_COVARIANCE in header
    assert '#define FLOW_STATS_EXTREMA %d' % _hip.STATS_EXTREMA in header
    # size_t strides: a store of more than 2^31 doubles is addressed
    assert _hip.SYMBOLS['flow_stats_update'][9] is ctypes.c_size_t
    assert _hip.SYMBOLS['flow_stats_merge'][8] is ctypes.c_size_t
    assert ctypes.sizeof(_hip.StatsFreq) == 8 + 2 * 8 * _hip.STATS_MAX_FREQ
    # argument checks that need no device: nothing to do, and bad arguments
    upd, mrg = lib.flow_stats_update, lib.flow_stats_merge
    assert upd(0, 1, 0, None, 1.0, 0.0, 0.0, None, None, 0, None) == 0
    assert upd(0, 2, 3, None, 1.0, 0.0, 0.0, None, None, 7, None) == 0
    assert mrg(0, 2, 3, 8, 0.5, 0.5, None, None, 0, None) == 0
    buf = (ctypes.c_double * 64)()
    base = ctypes.addressof(buf)
    base += (16 - base % 16) % 16
    p = ctypes.c_void_p(base)                   # the planes: 16-byte aligned
    x = ctypes.c_void_p(base + 8 * 40)          # 5 doubles behind 4 planes of 6
    assert upd(5, 1, 0, None, 1.0, 0.0, 0.0, x, p, 5, None) == 2     # odd ld
    assert b'ld' in lib.flow_last_error()
    assert upd(5, 1, 0, None, 1.0, 0.0, 0.0, x, p, 4, None) == 2     # ld < n
    assert b'ld' in lib.flow_last_error()
    assert upd(5, 1, 0, None, 1.0, 0.0, 0.0, x, None, 6, None) == 2
    assert upd(5, 1, 0, None, 1.0, 0.0, 0.0, None, p, 6, None) == 2
    assert b'pointers' in lib.flow_last_error()
    freq = _hip.StatsFreq()
    freq.n = 9
    assert upd(5, 1, 0, ctypes.byref(freq), 1.0, 0.0, 0.0, x, p, 6, None) == 2
    assert b'FLOW_STATS_MAX_FREQ' in lib.flow_last_error()
    assert upd(5, 3, 0, None, 1.0, 0.0, 0.0, x, p, 6, None) == 2     # dim
    assert upd(5, 1, 4, None, 1.0, 0.0, 0.0, x, p, 6, None) == 2     # flags
    assert upd(-1, 1, 0, None, 1.0, 0.0, 0.0, x, p, 6, None) == 2
    assert upd(5, 1, 0, None, 1.0, 0.0, 0.0, p, p, 6, None) == 2
    assert b'overlaps' in lib.flow_last_error()
    assert upd(5, 1, 0, None, 1.0, 0.0, 0.0, x,
               ctypes.c_void_p(base + 8), 6, None) == 2
    assert b'aligned' in lib.flow_last_error()
    q = ctypes.c_void_p(base + 8 * 32)
    assert mrg(5, 1, 1, 0, 0.5, 0.5, p, q, 5, None) == 2             # odd ld
    assert mrg(5, 1, 1, 0, 0.5, 0.5, p, q, 4, None) == 2             # ld < n
    assert mrg(5, 1, 1, 9, 0.5, 0.5, p, q, 6, None) == 2
    assert b'FLOW_STATS_MAX_FREQ' in lib.flow_last_error()
    assert mrg(5, 1, 1, 0, 0.5, 0.5, None, q, 6, None) == 2
    assert mrg(5, 1, 1, 0, 0.5, 0.5, p, None, 6, None) == 2
    assert mrg(5, 1, 1, 0, 0.5, 0.5, p, p, 6, None) == 2
    assert b'overlap' in lib.flow_last_error()


# -- the restatement against the long-double reference -------------------------------------
@pytest.mark.parametrize('dim', [1, 2])
def test_restatement_against_two_pass(dim):
    n = 37
    X, w, t = stref.samples(K, dim, n, seed=dim)
    R = Restatement(dim, n, True, FREQS8, True)
    for j in range(K):
        R.update(X[j], w[j], t[j])
    assert R.count == K
    worst = stref.compare(R, X, w, t, FREQS8, True, True,
                          'restatement x%d' % dim)
    assert worst <= 1.0


def test_restatement_exact_cases():
    dim, n = 2, 37
    X, w, t = stref.samples(K, dim, n, seed=5)
    # the first update: mean == x bit for bit, M2 == 0.0
    R = Restatement(dim, n, True, FREQS8[:2], True)
    R.update(X[0], w[0], t[0])
    assert numpy.array_equal(_bits(R.mean), _bits(X[0]))
    assert (R.M2 == 0.0).all() and not numpy.signbit(R.M2).any()
    assert numpy.array_equal(R.min, X[0]) and numpy.array_equal(R.max, X[0])
    assert (R.tmin == t[0]).all() and (R.tmax == t[0]).all()
    # a constant sequence: the mean stays, M2 stays 0.0 exactly
    R = Restatement(dim, n, True, (), True)
    for j in range(K):
        R.update(X[3], w[j], t[j])
    assert numpy.array_equal(_bits(R.mean), _bits(X[3]))
    assert (R.M2 == 0.0).all()
    assert (R.tmin == t[0]).all() and (R.tmax == t[0]).all()   # the first stays


def test_restatement_merge_and_state():
    dim, n, K = 2, 37, 20              # unfused halves: k >= 19
    X, w, t = stref.samples(K, dim, n, seed=9)
    assert FREQS8[2] * t[-1] <= K

    def run(js):
        R = Restatement(dim, n, True, FREQS8[:3], True)
        for j in js:
            R.update(X[j], w[j], t[j])
        return R
    whole, a, b = run(range(K)), run(range(K // 2)), run(range(K // 2, K))
    # merging with an empty object, both ways: bit for bit
    before = a.stacked().copy()
    a.merge(Restatement(dim, n, True, FREQS8[:3], True))
    assert numpy.array_equal(_bits(a.stacked()), _bits(before))
    assert a.count == K // 2
    empty = Restatement(dim, n, True, FREQS8[:3], True)
    empty.merge(a)
    assert numpy.array_equal(_bits(empty.stacked()), _bits(before))
    assert (empty.W, empty.count) == (a.W, a.count)
    # halves against the whole: within the bounds of the reference, and as
    # close to the uninterrupted run
    a.merge(b)
    assert a.count == K and abs(a.W - whole.W) <= 2 * EPS * whole.W
    worst = stref.compare(a, X, w, t, FREQS8[:3], True, True, 'merged halves',
                          min_k=19)
    assert worst <= 1.0
    # a state() / from_state round trip on arrays, then continued updates
    half = run(range(K // 2))
    back = Restatement.from_state(dim, n, True, FREQS8[:3], True, half.state())
    for j in range(K // 2, K):
        back.update(X[j], w[j], t[j])
    assert numpy.array_equal(_bits(back.stacked()), _bits(whole.stacked()))
    assert (back.W, back.count) == (whole.W, whole.count)
    with pytest.raises(ValueError, match='state'):
        Restatement.from_state(1, n, True, FREQS8[:3], True, half.state())


# -- the Fourier identity -----------------------------------------------------------------
COEF = numpy.array([   # m, a, b, c per entry
    [0.3, 1.0, 0.5, 0.25], [-2.0, 0.7, -1.1, 0.4], [0.0, 0.0, 1.0, -0.6]])


def test_fourier_identity_on_the_restatement():
    X, w, t, freqs, D = stref.fourier_identity_samples(COEF)
    assert D <= EPS * numpy.abs(X).max()
    stref.check_preconditions(len(w), t, freqs)
    R = Restatement(1, 3, True, freqs, False)
    for j in range(len(w)):
        R.update(X[j], w[j], t[j])
    stref.fourier_identity_check(
        'restatement', R.mean[0], R.M2[0] / R.W,
        (2.0 / R.W * R.A[0, 0], 2.0 / R.W * R.B[0, 0]),
        (2.0 / R.W * R.A[1, 0], 2.0 / R.W * R.B[1, 0]), X, w, D, COEF)
