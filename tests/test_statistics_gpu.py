# -*- coding: utf-8 -*-
'''
fem.Statistics on the HIP path (flow_amd/fem/statistics.py; csrc/
stats_kernels.hip): the two kernels on raw stores and the class end to end,
against the long-double two-pass reference of tests/statistics_reference.py
(never against the code under test).  Every test prints its measured error
next to its bound (pytest -s).

The bound: error <= C k eps scale per entry, C = 5, k the number of samples,
eps = 2^-52 (u = eps / 2 is one rounding), with the scales

    mean           X_i = max_j |x_ji|
    M2_ab          Q = sum_j w_j (|x_ja| + X_a) (|x_jb| + X_b)
                   (a = b: sum_j w_j (|x_ji| + max_j |x_ji|)^2)
    Fourier sums   F = sum_j w_j |x_ji|
    extrema and their times: exact.

Derivation (first order in u).  The roundings of one update are counted as
the kernel header writes it; p = 0 for the device, whose fma rounds once, and
p = 1 for the numpy restatement of the host test, which writes c + a * b and
rounds twice, so that the same C covers both.  The host keeps W_j = fl(W_j-1 +
w_j): relative error (j - 1) u.

Mean.  m_j = m_j-1 + r_j (x_j - m_j-1), r_j = w_j / W_j.  Roundings: delta
(1), the fma (1 + p); r_j carries j u (the sum and the division).  With
|x - m| <= 2 X and |m| <= X the error made in step j is at most r_j 2 X
(j + 1 + p) u + X u; it reaches the end multiplied by prod_i>j (1 - r_i) =
W_j / W_k <= 1, its first part therefore by w_j / W_k, and sum_j w_j = W_k:
    |e_k| <= 2 X (k + 1 + p) u + k X u = (3 k + 2 + 2 p) X u.
M2.  M_j = M_j-1 + s_j delta_a delta_b, s_j = w_j W_j-1 / W_j <= w_j and
|delta| <= |x| + X, so sum_j s_j |delta_a delta_b| <= Q and so is every
partial sum.  The fma's roundings: k u Q.  The relative error of a term: s_j
carries (2 j - 1) u (two sums, a product, a division), the two deltas 2 u,
s * delta 1 u, the unfused product p u: (2 k + 2 + p) u Q.  The error e_j-1
<= (3 k - 1 + 2 p) X u of the mean inside both deltas: s_j (|delta_a| X_b +
|delta_b| X_a) |e| / X <= 2 (3 k - 1 + 2 p) u Q.  Together
    (9 k + 5 p) u Q = (4.5 k + 2.5 p) eps Q.
Fourier.  The phase 2 pi fmod(f t, 1): fl(f t) is off by f |t| u cycles, fmod
is exact, the constant 2 pi and the product with it 2 u of at most 2 pi:
2 pi (f |t| + 2) u; cos and sin 2 u more, the product with w 1 u: a
coefficient is within w (2 pi f |t| + 4 pi + 3) u.  The fma adds (1 + p) u F
per step:
    ((1 + p) k + 2 pi f |t| + 15.6) u F <= (1 + pi + 7.8 / k) k eps F
for f |t| <= k, which is below 5 k eps F from k = 10 on.
Merge (Chan), two halves of k / 2 updates against the whole: q = Wb / W
carries k u, g = Wa Wb / W 1.5 k u, and g d_a d_b <= (W / 4) (2 X_a) (2 X_b)
<= Q.  Mean: the halves' (1.5 k + 2 + 2 p) X u, 2 X (k + 1 + p) u for the
term and X u for the sum: (3.5 k + 5 + 4 p) X u.  M2: the halves' (4.5 k +
5 p) u Q; the term (1.5 k + 3 + p) u Q; the means' errors inside d,
g 4 X (3 k + 4 + 4 p) X u <= (3 k + 4 + 4 p) u Q; the two additions 2 u Q:
    (9 k + 9 + 10 p) u Q = (4.5 k + 4.5 + 5 p) eps Q,
below 5 k eps Q from k = 9 on for the device and from k = 19 on for the
restatement (the host test merges halves of k = 20 samples).

So C = 5 (the largest of 1.5 + 2 / k, 4.5 + 2.5 / k and 1 + pi + 7.8 / k,
rounded up) for k >= 10 updates, k >= 9 (19 unfused) merged, and f |t| <= k:
statistics_reference.check_preconditions asserts that of every test's inputs.
The getters add the rounding of W ((k - 1) u) and at most three roundings of
the finishing arithmetic, k eps of the result in all: the end-to-end tests
hold variance, covariance, tke and fourier against (C k + k) eps scale / W
(times 2 for fourier); mean and the extrema are copies.

Measured on the MI355X, as the largest error / bound over all cases: mean
0.016, M2 0.0067, Fourier sums 0.10 (n = 4099, f = 0.6, where the phase term
of the derivation is largest), merged halves 0.10, the getters 0.029.

Sizes of the raw tests: n = 1, 2 (one lane), 255, 257 (less and more than a
wave's worth of pairs), 513 (odd, just past the 256 pair-lanes of one block),
4099 (odd, several blocks).  The padding of every plane is NaN before the
calls and must be NaN after them.  For dim = 2 x is laid out as Function.data
is (component 1 at x + n): with an odd n it is 8 bytes off a 16-byte boundary;
the samples lie back to back in one tensor, so with an odd dim * n every
second sample has its FIRST component off instead.
'''
import ctypes
import functools

import numpy
import pytest

from flow_amd import _hip, device, fem

import recovery_reference as rref
import statistics_reference as stref
from statistics_reference import C_BOUND, EPS, Restatement

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 255, 257, 513, 4099]
K = 12
FREQS8 = (0.05, 0.11, 0.17, 0.23, 0.31, 0.4, 0.5, 0.6)     # f t <= 0.6 * 18 < K
OPTIONS = [(False, False), (True, False), (False, True), (True, True)]


def _bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.int64)


def _ld(n):
    return (n + 3) & ~1          # even and > n: every plane has padding


def _nplanes(dim, cov, nf, ext):
    return dim + (cov * (1 if dim == 1 else 3)) + 2 * dim * nf + 4 * dim * ext


@functools.lru_cache(maxsize=4)
def _samples(dim, n):
    '''(X, w, t, the samples back to back on the device).'''
    X, w, t = stref.samples(K, dim, n, seed=10 * n + dim)
    return X, w, t, device.to_device(X.reshape(-1))


def _fresh(dim, n, cov, nf, ext):
    '''A reset store on the device with NaN padding.'''
    ld = _ld(n)
    P = numpy.full((_nplanes(dim, cov, nf, ext), ld), numpy.nan)
    P[:, :n] = Restatement(dim, n, cov, FREQS8[:nf], ext).stacked()
    return device.to_device(P.reshape(-1))


def _update(lib, Pd, dim, n, cov, nf, ext, xd, W, w, t):
    '''One flow_stats_update with the host scalars of the definitions; the new
    weight.'''
    W1 = W + w
    freq = _hip.StatsFreq()
    freq.n = nf
    for i, f in enumerate(FREQS8[:nf]):
        phi = (2.0 * numpy.pi) * numpy.fmod(f * t, 1.0)
        freq.c[i], freq.s[i] = w * numpy.cos(phi), -(w * numpy.sin(phi))
    _hip.check(lib.flow_stats_update(
        n, dim, cov * 1 + ext * 2, ctypes.byref(freq), w / W1, (w * W) / W1, t,
        _hip.f64(xd, dim * n), _hip.f64(Pd, _nplanes(dim, cov, nf, ext) * _ld(n)),
        _ld(n), _hip.stream()))
    return W1


def _run(lib, dim, n, cov, nf, ext, js, Pd=None):
    '''The updates js of the samples into a fresh store (or Pd): (store, W).'''
    X, w, t, Xd = _samples(dim, n)
    Pd = _fresh(dim, n, cov, nf, ext) if Pd is None else Pd
    W = 0.0
    for j in js:
        W = _update(lib, Pd, dim, n, cov, nf, ext,
                    Xd[j * dim * n:(j + 1) * dim * n], W, float(w[j]), float(t[j]))
    return Pd, W


def _read(Pd, dim, n, cov, nf, ext, W=0.0, count=0):
    '''(planes (P, n), the same as a Restatement); the padding must be NaN.'''
    P = device.to_host(Pd).numpy().reshape(-1, _ld(n))
    assert numpy.isnan(P[:, n:]).all(), 'the padding was written'
    planes = P[:, :n].copy()
    return planes, Restatement.from_state(
        dim, n, cov, FREQS8[:nf], ext,
        {'planes': planes, 'weight': W, 'count': count})


# -- 1. flow_stats_update ------------------------------------------------------------------
@pytest.mark.parametrize('cov,ext', OPTIONS)
@pytest.mark.parametrize('nf', [0, 1, 8])
@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('n', SIZES)
def test_update_against_two_pass(hip, n, dim, nf, cov, ext):
    X, w, t, Xd = _samples(dim, n)
    tag = 'n %d x%d nf %d cov %d ext %d' % (n, dim, nf, cov, ext)
    before = _hip.launch_count()
    Pd, W = _run(hip, dim, n, cov, nf, ext, range(K))
    assert _hip.launch_count() == before + K          # one launch per update
    planes, got = _read(Pd, dim, n, cov, nf, ext, W, K)
    worst = stref.compare(got, X, w, t, FREQS8[:nf], cov, ext, tag)
    assert worst <= 1.0
    # two identical sequences of calls: the same bits
    Pd2, _ = _run(hip, dim, n, cov, nf, ext, range(K))
    again, _ = _read(Pd2, dim, n, cov, nf, ext)
    assert numpy.array_equal(_bits(planes), _bits(again)), tag


@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('n', SIZES)
def test_update_exact_cases(hip, n, dim):
    X, w, t, Xd = _samples(dim, n)
    cov, nf, ext = True, 1, True
    # the first update: mean == x bit for bit, M2 == 0.0, the extrema are x
    Pd, W = _run(hip, dim, n, cov, nf, ext, [0])
    _, got = _read(Pd, dim, n, cov, nf, ext)
    assert numpy.array_equal(_bits(got.mean), _bits(X[0]))
    assert (got.M2 == 0.0).all()
    assert numpy.array_equal(got.min, X[0]) and numpy.array_equal(got.max, X[0])
    assert (got.tmin == t[0]).all() and (got.tmax == t[0]).all()
    # a constant field: the mean stays, M2 stays 0.0, the first time stays
    Pd = _fresh(dim, n, cov, nf, ext)
    W = 0.0
    for j in range(K):
        W = _update(hip, Pd, dim, n, cov, nf, ext, Xd[3 * dim * n:4 * dim * n],
                    W, float(w[j]), float(t[j]))
    _, got = _read(Pd, dim, n, cov, nf, ext)
    assert numpy.array_equal(_bits(got.mean), _bits(X[3]))
    assert (got.M2 == 0.0).all()
    assert (got.tmin == t[0]).all() and (got.tmax == t[0]).all()
    print('n %d x%d: first update and constant field exact' % (n, dim))


def test_update_nothing_to_do_and_refusals(hip):
    X, w, t, Xd = _samples(1, 255)
    Pd = _fresh(1, 255, True, 0, False)
    keep = device.to_host(Pd).numpy().copy()
    before = _hip.launch_count()
    args = (None, 1.0, 0.0, 0.0, _hip.f64(Xd), _hip.f64(Pd))
    assert hip.flow_stats_update(0, 1, 1, *args, 258, _hip.stream()) == 0
    assert hip.flow_stats_merge(0, 1, 1, 0, 0.5, 0.5, _hip.f64(Pd),
                                _hip.f64(Xd), 258, _hip.stream()) == 0
    for ld in (257, 254):
        with pytest.raises(ValueError, match='ld'):
            _hip.check(hip.flow_stats_update(255, 1, 1, *args, ld,
                                             _hip.stream()))
    with pytest.raises(ValueError, match='aligned'):
        _hip.check(hip.flow_stats_update(
            200, 1, 1, *args[:5], ctypes.c_void_p(Pd.data_ptr() + 8), 258,
            _hip.stream()))
    with pytest.raises(ValueError, match='overlaps'):
        _hip.check(hip.flow_stats_update(
            255, 1, 1, *args[:4], _hip.f64(Pd[258:]), _hip.f64(Pd), 258,
            _hip.stream()))
    assert _hip.launch_count() == before
    assert numpy.array_equal(_bits(device.to_host(Pd).numpy()), _bits(keep))


# -- 2. flow_stats_merge -------------------------------------------------------------------
def _merge(lib, Pa, Pb, dim, n, cov, nf, ext, Wa, Wb):
    W = Wa + Wb
    np_ = _nplanes(dim, cov, nf, ext) * _ld(n)
    _hip.check(lib.flow_stats_merge(
        n, dim, cov * 1 + ext * 2, nf, Wb / W, (Wa * Wb) / W,
        _hip.f64(Pa, np_), _hip.f64(Pb, np_), _ld(n), _hip.stream()))
    return W


@pytest.mark.parametrize('cov,nf,ext', [(True, 2, True), (False, 0, False),
                                        (True, 8, False)])
@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('n', SIZES)
def test_merge_halves_against_the_whole(hip, n, dim, cov, nf, ext):
    X, w, t, Xd = _samples(dim, n)
    tag = 'merge n %d x%d nf %d cov %d ext %d' % (n, dim, nf, cov, ext)
    Pa, Wa = _run(hip, dim, n, cov, nf, ext, range(K // 2))
    Pb, Wb = _run(hip, dim, n, cov, nf, ext, range(K // 2, K))
    keep_b = device.to_host(Pb).numpy().copy()
    # an empty other: bit for bit
    keep_a, _ = _read(Pa, dim, n, cov, nf, ext)
    before = _hip.launch_count()
    _hip.check(hip.flow_stats_merge(
        n, dim, cov * 1 + ext * 2, nf, 0.0, 0.0, _hip.f64(Pa),
        _hip.f64(_fresh(dim, n, cov, nf, ext)), _ld(n), _hip.stream()))
    assert _hip.launch_count() == before + 1
    same, _ = _read(Pa, dim, n, cov, nf, ext)
    assert numpy.array_equal(_bits(same), _bits(keep_a)), tag
    # the halves
    W = _merge(hip, Pa, Pb, dim, n, cov, nf, ext, Wa, Wb)
    _, got = _read(Pa, dim, n, cov, nf, ext, W, K)
    worst = stref.compare(got, X, w, t, FREQS8[:nf], cov, ext, tag, min_k=9)
    assert worst <= 1.0
    # the other store is only read
    assert numpy.array_equal(_bits(device.to_host(Pb).numpy()), _bits(keep_b))


@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('n', [1, 257, 4099])
def test_merge_extrema_ties_keep_self(hip, n, dim):
    '''Both stores saw the same fields, self at the times t, other at t + 100:
    every extremum ties and self's times stay; then other holds a strictly
    lower minimum at one entry only, and only that entry changes hands.'''
    X, w, t, Xd = _samples(dim, n)
    cov, nf, ext = False, 0, True
    Pa, Wa = _run(hip, dim, n, cov, nf, ext, range(4))
    Pb = _fresh(dim, n, cov, nf, ext)
    Wb = 0.0
    for j in range(4):
        Wb = _update(hip, Pb, dim, n, cov, nf, ext,
                     Xd[j * dim * n:(j + 1) * dim * n], Wb, float(w[j]),
                     float(t[j]) + 100.0)
    low = X[0].reshape(-1).copy()            # sample 0 again: more ties ...
    low[0] = -2.0                            # ... but for one entry
    Wb = _update(hip, Pb, dim, n, cov, nf, ext, device.to_device(low), Wb, 1.0,
                 300.0)
    keep, _ = _read(Pa, dim, n, cov, nf, ext)
    _merge(hip, Pa, Pb, dim, n, cov, nf, ext, Wa, Wb)
    planes, got = _read(Pa, dim, n, cov, nf, ext)
    want = Restatement.from_state(dim, n, cov, (), ext,
                                  {'planes': keep, 'weight': 0, 'count': 0})
    want.min[0, 0], want.tmin[0, 0] = -2.0, 300.0
    for name in ('min', 'max', 'tmin', 'tmax'):
        assert numpy.array_equal(getattr(got, name), getattr(want, name)), name
    print('merge n %d x%d: ties keep self' % (n, dim))


# -- 3. fem.Statistics end to end --------------------------------------------------------------
FREQS = (2.0, 5.0)


def _field(j):
    return [lambda x, y: numpy.sin(3 * x + 0.7 * j) * numpy.exp(y) + 0.1 * j,
            lambda x, y: numpy.cos(2 * y - x + 0.4 * j) - 0.05 * j * j * x]


DT = numpy.array([0.02 * (1.0 + 0.5 * numpy.sin(1.3 * j)) for j in range(K)])
T = numpy.cumsum(DT)                         # <= 0.36: f t <= 1.8


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return fem.UnitSquareMesh(4, 4) if name == 'square 4' \
        else fem.karman_channel(60, 14, fitted=True)


@functools.lru_cache(maxsize=None)
def _fields(name, deg, dim):
    V = fem.FunctionSpace(_mesh(name), 'CG', deg, dim=dim)
    us = [rref.field(V, _field(j)[:dim]) for j in range(K)]
    X = numpy.array([u.array().reshape(dim, V.N) for u in us])
    X.flags.writeable = False
    return V, us, X


def _forbid(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError('update moved data between host and device')
    monkeypatch.setattr(device, 'to_device', refuse)
    monkeypatch.setattr(device, 'to_host', refuse)


def _as_restatement(S):
    st = S.state()
    return st, Restatement.from_state(
        S.V.dim, S.N, S.covariance_kept, S.frequencies, S.extrema, st)


def _hold(what, got, want, bound):
    err = numpy.abs(got.astype(stref.LD) - want).astype(float)
    ok = bound > 0
    ratio = (err[ok] / bound[ok]).max() if ok.any() else 0.0
    print('%s: error %.2e  bound %.2e  (largest error / bound %.2e)'
          % (what, err.max(), bound.max(), ratio))
    assert numpy.isfinite(err).all() and (err <= bound).all(), what


@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('deg', [1, 2])
@pytest.mark.parametrize('name', ['square 4', 'fitted channel'])
def test_statistics_against_two_pass(hip, monkeypatch, name, deg, dim):
    V, us, X = _fields(name, deg, dim)
    N = V.N
    tag = '%s P%d x%d' % (name, deg, dim)
    S = fem.Statistics(V, covariance=True, frequencies=FREQS, extrema=True)
    before = _hip.launch_count()
    with monkeypatch.context() as m:
        _forbid(m)
        for j, u in enumerate(us):
            S.update(u, dt=DT[j], t=T[j])
    assert _hip.launch_count() == before + K          # one launch per update
    assert S.count == K and S.t_first == T[0] and S.t_last == T[-1]
    assert abs(S.weight - DT.sum()) <= K * EPS * DT.sum()
    st, got = _as_restatement(S)
    assert stref.compare(got, X, DT, T, FREQS, True, True, tag) <= 1.0
    # the getters: copies of the planes, or the planes scaled
    ref = stref.two_pass(X, DT, T, FREQS)
    sc = stref.scales(X, DT)
    Wl = ref['W']
    unit = (C_BOUND * K + K) * EPS
    mean = S.mean()
    assert isinstance(mean, fem.Function) and mean.function_space().same_as(V)
    assert numpy.array_equal(_bits(mean.array()), _bits(got.mean.reshape(-1)))
    out = fem.Function(V)
    assert S.mean(out=out) is out
    assert numpy.array_equal(_bits(out.array()), _bits(mean.array()))
    diag = [0] if dim == 1 else [0, 2]
    var = S.variance().array().reshape(dim, N)
    _hold(tag + ' variance', var, ref['M2'][diag] / Wl,
          unit * sc['M2'][diag] / float(Wl))
    assert (var >= 0.0).all()
    rms = S.rms(out=out).array().reshape(dim, N)
    assert numpy.isfinite(rms).all() and (rms >= 0.0).all()
    # sqrt is correctly rounded: rms^2 is within 3 roundings of the variance
    assert (numpy.abs(rms * rms - var) <= 2 * EPS * var).all()
    cov = S.covariance()
    assert len(cov) == (1 if dim == 1 else 3)
    for p, f in enumerate(cov):
        assert f.function_space().same_as(S.scalar_space)
        _hold(tag + ' covariance %d' % p, f.array(), ref['M2'][p] / Wl,
              unit * sc['M2'][p] / float(Wl))
    if dim == 2:
        assert S.scalar_space.dim == 1 and S.scalar_space.degree == deg
        _hold(tag + ' tke', S.tke().array(),
              (ref['M2'][0] + ref['M2'][2]) / (2 * Wl),
              unit * (sc['M2'][0] + sc['M2'][2]) / (2 * float(Wl)))
    else:
        with pytest.raises(ValueError, match='2-vector'):
            S.tke()
    for i in range(len(FREQS)):
        re, im = S.fourier(i)
        _hold(tag + ' fourier %d re' % i, re.array().reshape(dim, N),
              2 * ref['A'][i] / Wl, 2 * unit * sc['fourier'] / float(Wl))
        _hold(tag + ' fourier %d im' % i, im.array().reshape(dim, N),
              2 * ref['B'][i] / Wl, 2 * unit * sc['fourier'] / float(Wl))
    for call, key in ((S.minimum, 'min'), (S.maximum, 'max'),
                      (S.time_of_minimum, 'tmin'), (S.time_of_maximum, 'tmax')):
        assert numpy.array_equal(call().array().reshape(dim, N), ref[key]), key
    # state() -> from_state -> continued updates: the uninterrupted run's bits
    half = fem.Statistics(V, covariance=True, frequencies=FREQS, extrema=True)
    for j in range(K // 2):
        half.update(us[j], dt=DT[j], t=T[j])
    back = fem.Statistics.from_state(V, half.state())
    for j in range(K // 2, K):
        back.update(us[j], dt=DT[j], t=T[j])
    assert numpy.array_equal(_bits(back.state()['planes']), _bits(st['planes']))
    assert (back.weight, back.count, back.t_first, back.t_last) \
        == (S.weight, S.count, S.t_first, S.t_last)
    # merge through the class: halves against the whole, an empty other, into
    # an empty self
    rest = fem.Statistics(V, covariance=True, frequencies=FREQS, extrema=True)
    for j in range(K // 2, K):
        rest.update(us[j], dt=DT[j], t=T[j])
    keep = half.state()['planes']
    half.merge(fem.Statistics(V, covariance=True, frequencies=FREQS,
                              extrema=True))
    assert numpy.array_equal(_bits(half.state()['planes']), _bits(keep))
    empty = fem.Statistics(V, covariance=True, frequencies=FREQS, extrema=True)
    empty.merge(half)
    assert numpy.array_equal(_bits(empty.state()['planes']), _bits(keep))
    assert (empty.weight, empty.count) == (half.weight, half.count)
    half.merge(rest)
    assert half.count == K and (half.t_first, half.t_last) == (T[0], T[-1])
    _, merged = _as_restatement(half)
    assert stref.compare(merged, X, DT, T, FREQS, True, True,
                         tag + ' merged', min_k=9) <= 1.0
    # reset()
    S.reset()
    assert S.weight == 0.0 and S.count == 0 and S.t_first is None
    with pytest.raises(ValueError, match='no samples'):
        S.mean()
    fresh = Restatement(dim, N, True, FREQS, True).stacked()
    assert numpy.array_equal(_bits(S.state()['planes']), _bits(fresh))
    S.update(us[2], dt=0.3, t=1.0)
    assert numpy.array_equal(_bits(S.mean().array()), _bits(us[2].array()))


def test_statistics_mean_only_and_no_time(hip, monkeypatch):
    '''covariance=False, no frequencies, no extrema: one plane per component,
    no t needed.'''
    V, us, X = _fields('square 4', 2, 2)
    S = fem.Statistics(V, covariance=False)
    assert S.planes == 2
    with monkeypatch.context() as m:
        _forbid(m)
        for j, u in enumerate(us):
            S.update(u, dt=DT[j])
    assert S.t_first is None and S.t_last is None
    _, got = _as_restatement(S)
    assert stref.compare(got, X, DT, None, (), False, False,
                         'mean only') <= 1.0
    with pytest.raises(ValueError, match='covariance=False'):
        S.variance()


def test_fourier_identity_through_update(hip):
    '''x = m + a cos wt + b sin wt + c cos 2wt over three periods of 16 equal
    steps: mean m, fourier(0) = (a, -b), fourier(1) = (c, 0), variance (a^2 +
    b^2 + c^2) / 2, with m, a, b, c varying over the nodes.'''
    V = fem.FunctionSpace(fem.UnitSquareMesh(4, 4), 'CG', 1)
    xy = V.layout.dof_coords
    coef = numpy.stack([1.0 + xy[:, 0], numpy.sin(3 * xy[:, 1]) + 0.2,
                        xy[:, 0] * xy[:, 1] - 0.3, 0.5 - xy[:, 1]], axis=1)
    X, w, t, freqs, D = stref.fourier_identity_samples(coef)
    stref.check_preconditions(len(w), t, freqs)
    S = fem.Statistics(V, frequencies=freqs)
    u = fem.Function(V)
    for j in range(len(w)):
        u.set_array(X[j, 0])
        S.update(u, dt=w[j], t=t[j])
    stref.fourier_identity_check(
        'Statistics', S.mean().array(), S.variance().array(),
        tuple(f.array() for f in S.fourier(0)),
        tuple(f.array() for f in S.fourier(1)), X, w, D, coef)
