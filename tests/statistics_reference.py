# -*- coding: utf-8 -*-
'''
Host references for fem.Statistics (flow_amd/fem/statistics.py; csrc/
stats_kernels.hip), independent of the package.

Restatement   update and merge in float64 numpy, the formulas of the kernel
              header in their order.  numpy has no fma: every fma(a, b, c) is
              written c + a * b, one rounding more than the kernel's (the
              derivation of the bound in tests/test_statistics_gpu.py counts
              it).  With a = 1 or a * b = 0 the two agree, so the exact cases
              (first update, constant field) hold here as on the device.
two_pass      the same statistics by their definitions in numpy.longdouble
              from the samples themselves: the weighted mean, the central
              second moments about THAT mean, the Fourier sums with the phase
              reduced in long double, the extrema with first-occurrence times.
scales        the per-entry scales the bounds are multiples of.

Samples: X (k, dim, n), weights w (k,), times t (k,).
'''
import math

import numpy

LD = numpy.longdouble
EPS = numpy.finfo(float).eps
# the constant of the bounds: derived in tests/test_statistics_gpu.py
C_BOUND = 5.0


def pairs(dim):
    '''The (a, b) of the M2 planes, in store order.'''
    return [(0, 0)] if dim == 1 else [(0, 0), (0, 1), (1, 1)]


class Restatement(object):
    '''The accumulators as numpy arrays: mean (dim, n), M2 (1 | 3, n) or None,
    A and B (nf, dim, n), min, max, tmin, tmax (dim, n) or None.'''

    def __init__(self, dim, n, covariance=True, frequencies=(), extrema=False):
        self.dim, self.n = dim, n
        self.covariance, self.extrema = bool(covariance), bool(extrema)
        self.frequencies = tuple(float(f) for f in frequencies)
        nf = len(self.frequencies)
        self.W, self.count = 0.0, 0
        self.mean = numpy.zeros((dim, n))
        self.M2 = numpy.zeros((len(pairs(dim)), n)) if covariance else None
        self.A = numpy.zeros((nf, dim, n))
        self.B = numpy.zeros((nf, dim, n))
        self.min = self.max = self.tmin = self.tmax = None
        if extrema:
            self.min = numpy.full((dim, n), numpy.inf)
            self.max = numpy.full((dim, n), -numpy.inf)
            self.tmin = numpy.full((dim, n), numpy.nan)
            self.tmax = numpy.full((dim, n), numpy.nan)

    def update(self, x, w, t=0.0):
        x = numpy.asarray(x, dtype=numpy.float64).reshape(self.dim, self.n)
        w, t, W = float(w), float(t), self.W
        W1 = W + w
        r = w / W1
        s = (w * W) / W1
        delta = x - self.mean
        self.mean = self.mean + r * delta
        if self.covariance:
            for p, (a, b) in enumerate(pairs(self.dim)):
                self.M2[p] = self.M2[p] + (s * delta[a]) * delta[b]
        for k, f in enumerate(self.frequencies):
            phi = (2.0 * math.pi) * math.fmod(f * t, 1.0)
            c, sn = w * math.cos(phi), -(w * math.sin(phi))
            self.A[k] = self.A[k] + c * x
            self.B[k] = self.B[k] + sn * x
        if self.extrema:
            lo = x < self.min
            self.min = numpy.where(lo, x, self.min)
            self.tmin = numpy.where(lo, t, self.tmin)
            hi = x > self.max
            self.max = numpy.where(hi, x, self.max)
            self.tmax = numpy.where(hi, t, self.tmax)
        self.W = W1
        self.count += 1

    def merge(self, other):
        assert (other.dim, other.n, other.covariance, other.extrema,
                other.frequencies) == (self.dim, self.n, self.covariance,
                                       self.extrema, self.frequencies)
        if other.W == 0.0:
            return
        if self.W == 0.0:
            for name in ('mean', 'M2', 'A', 'B', 'min', 'max', 'tmin', 'tmax'):
                v = getattr(other, name)
                setattr(self, name, None if v is None else v.copy())
            self.W, self.count = other.W, other.count
            return
        Wa, Wb = self.W, other.W
        W = Wa + Wb
        q = Wb / W
        g = (Wa * Wb) / W
        d = other.mean - self.mean
        self.mean = self.mean + q * d
        if self.covariance:
            for p, (a, b) in enumerate(pairs(self.dim)):
                self.M2[p] = (self.M2[p] + other.M2[p]) + (g * d[a]) * d[b]
        self.A = self.A + other.A
        self.B = self.B + other.B
        if self.extrema:
            lo = other.min < self.min
            self.min = numpy.where(lo, other.min, self.min)
            self.tmin = numpy.where(lo, other.tmin, self.tmin)
            hi = other.max > self.max
            self.max = numpy.where(hi, other.max, self.max)
            self.tmax = numpy.where(hi, other.tmax, self.tmax)
        self.W = W
        self.count += other.count

    def stacked(self):
        '''The planes in the order of the device store: (planes, n).'''
        rows = [self.mean]
        if self.covariance:
            rows.append(self.M2)
        for k in range(len(self.frequencies)):
            rows += [self.A[k], self.B[k]]
        if self.extrema:
            rows += [self.min, self.max, self.tmin, self.tmax]
        return numpy.concatenate(rows, axis=0)

    def state(self):
        return {'planes': self.stacked().copy(), 'weight': self.W,
                'count': self.count}

    @classmethod
    def from_state(cls, dim, n, covariance, frequencies, extrema, state):
        S = cls(dim, n, covariance, frequencies, extrema)
        P = numpy.asarray(state['planes'], dtype=numpy.float64)
        if P.shape != S.stacked().shape:
            raise ValueError('state: planes %r' % (P.shape,))
        at = dim
        S.mean = P[:dim].copy()
        if covariance:
            m = len(pairs(dim))
            S.M2 = P[at:at + m].copy()
            at += m
        for k in range(len(S.frequencies)):
            S.A[k] = P[at:at + dim]
            S.B[k] = P[at + dim:at + 2 * dim]
            at += 2 * dim
        if extrema:
            S.min, S.max, S.tmin, S.tmax = (
                P[at + j * dim:at + (j + 1) * dim].copy() for j in range(4))
        S.W, S.count = float(state['weight']), int(state['count'])
        return S


def two_pass(X, w, t=None, frequencies=()):
    '''The statistics of the samples by definition, in long double: a dict
    with W, mean (dim, n), M2 (1 | 3, n), A and B (nf, dim, n) as long double
    arrays and min, max, tmin, tmax (dim, n) as float64.'''
    X = numpy.asarray(X, dtype=numpy.float64)
    k, dim, n = X.shape
    Xl = X.astype(LD)
    wl = numpy.asarray(w, dtype=numpy.float64).astype(LD)
    W = wl.sum()
    mean = numpy.einsum('j,jan->an', wl, Xl) / W
    dev = Xl - mean
    M2 = numpy.array([numpy.einsum('j,jn,jn->n', wl, dev[:, a], dev[:, b])
                      for a, b in pairs(dim)])
    out = {'W': W, 'mean': mean, 'M2': M2}
    nf = len(frequencies)
    A = numpy.zeros((nf, dim, n), dtype=LD)
    B = numpy.zeros((nf, dim, n), dtype=LD)
    if nf:
        tl = numpy.asarray(t, dtype=numpy.float64).astype(LD)
        two_pi = 8 * numpy.arctan(LD(1))
        for i, f in enumerate(frequencies):
            phi = two_pi * numpy.fmod(LD(float(f)) * tl, LD(1))
            A[i] = numpy.einsum('j,jan->an', wl * numpy.cos(phi), Xl)
            B[i] = numpy.einsum('j,jan->an', -wl * numpy.sin(phi), Xl)
    out['A'], out['B'] = A, B
    if t is not None:
        tt = numpy.asarray(t, dtype=numpy.float64)
        out['min'], out['max'] = X.min(axis=0), X.max(axis=0)
        # argmin / argmax return the FIRST occurrence
        out['tmin'] = tt[X.argmin(axis=0)]
        out['tmax'] = tt[X.argmax(axis=0)]
    return out


def scales(X, w):
    '''Per entry: mean max_j |x|, (dim, n); M2 sum_j w_j (|x_a| + max |x_a|)
    (|x_b| + max |x_b|), (1 | 3, n) -- for a = b the sum_j w_j (|x_ji| + max_j
    |x_ji|)^2 of the issue; Fourier sum_j w_j |x|, (dim, n).'''
    X = numpy.abs(numpy.asarray(X, dtype=numpy.float64))
    w = numpy.asarray(w, dtype=numpy.float64)
    k, dim, n = X.shape
    top = X.max(axis=0)
    Y = X + top
    M2 = numpy.array([numpy.einsum('j,jn,jn->n', w, Y[:, a], Y[:, b])
                      for a, b in pairs(dim)])
    return {'mean': top, 'M2': M2,
            'fourier': numpy.einsum('j,jan->an', w, X)}


def check_preconditions(k, t, frequencies, min_k=10):
    '''What the derivation of C_BOUND assumes of a test's inputs: k >= 10
    updates (merged halves: k >= 9 with the device's fma, k >= 19 unfused)
    and f |t| <= k.'''
    assert k >= min_k
    if len(frequencies):
        assert max(frequencies) * numpy.abs(numpy.asarray(t)).max() <= k


def compare(got, X, w, t, frequencies, covariance, extrema, what, min_k=10):
    '''Hold the accumulators `got` (an object with mean, M2, A, B, min, ...
    as arrays, e.g. a Restatement) against two_pass within C_BOUND k eps
    scale per entry; the extrema and their times exactly.  Prints every
    measured error next to its bound; returns the largest error / bound.'''
    X = numpy.asarray(X, dtype=numpy.float64)
    k = X.shape[0]
    check_preconditions(k, t if t is not None else [0.0], frequencies, min_k)
    ref = two_pass(X, w, t, frequencies)
    sc = scales(X, w)
    unit = C_BOUND * k * EPS
    worst = 0.0

    def hold(name, value, want, scale):
        err = numpy.abs(value.astype(LD) - want).astype(float)
        bound = unit * scale
        assert numpy.isfinite(err).all(), (what, name)
        ratio = (err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() \
            else 0.0
        print('%s %s: error %.2e  bound %.2e  (largest error / bound %.2e)'
              % (what, name, err.max(), bound.max(), ratio))
        assert (err <= bound).all(), (what, name, ratio)
        return ratio

    worst = max(worst, hold('mean', got.mean, ref['mean'], sc['mean']))
    if covariance:
        worst = max(worst, hold('M2', got.M2, ref['M2'], sc['M2']))
        n_diag = [0] if X.shape[1] == 1 else [0, 2]
        assert (got.M2[n_diag] >= 0.0).all(), (what, 'negative M2')
    for i in range(len(frequencies)):
        worst = max(worst, hold('A[%d]' % i, got.A[i], ref['A'][i],
                                sc['fourier']))
        worst = max(worst, hold('B[%d]' % i, got.B[i], ref['B'][i],
                                sc['fourier']))
    if extrema:
        for name in ('min', 'max', 'tmin', 'tmax'):
            same = numpy.array_equal(getattr(got, name), ref[name])
            print('%s %s: %s' % (what, name, 'exact' if same else 'DIFFERS'))
            assert same, (what, name)
    return worst


def samples(k, dim, n, seed):
    '''k random samples in [-1, 1], unequal weights in [0.5, 1.5] and the
    times they end at (t_j = w_0 + ... + w_j <= 1.5 k).'''
    rng = numpy.random.RandomState(seed)
    X = rng.uniform(-1.0, 1.0, size=(k, dim, n))
    w = rng.uniform(0.5, 1.5, size=k)
    t = numpy.cumsum(w)
    for a in (X, w, t):
        a.flags.writeable = False
    return X, w, t


# -- the Fourier identity -----------------------------------------------------------------
PERIOD = 0.5           # a power of two: t_j = j T / 16 and f t_j are exact


def fourier_identity_samples(coef):
    '''x_j = m + a cos wt_j + b sin wt_j + c cos 2wt_j at t_j = j T / 16, j <
    48 (three periods), equal weights, evaluated in long double and rounded
    to double; coef (n, 4): m, a, b, c per entry.  Returns X (48, 1, n), w, t,
    the frequencies (1 / T, 2 / T) and D, the largest rounding of an x.'''
    coef = numpy.asarray(coef, dtype=numpy.float64)
    j = numpy.arange(48)
    t = j * PERIOD / 16.0
    ang = (8 * numpy.arctan(LD(1))) * (j % 16).astype(LD) / 16
    m, a, b, c = (coef[:, i].astype(LD)[None, :] for i in range(4))
    xl = m + a * numpy.cos(ang)[:, None] + b * numpy.sin(ang)[:, None] \
        + c * numpy.cos(2 * ang)[:, None]
    X = xl.astype(numpy.float64)
    D = float(numpy.abs(X.astype(LD) - xl).max())
    return X[:, None, :], numpy.full(48, PERIOD / 16.0), t, \
        (1.0 / PERIOD, 2.0 / PERIOD), D


def fourier_identity_check(what, mean, var, f0, f1, X, w, D, coef):
    '''mean, var (n,) and f0 = (re, im), f1 = (re, im) of the sequence above
    against m, (a^2 + b^2 + c^2) / 2, (a, -b), (c, 0).  The bound: C k eps
    scale for the accumulators (divided by W, times 2 for the Fourier modes),
    k eps of the result for the finishing arithmetic and the rounding of W,
    and what the rounding D of the samples can move the exact statistics by:
    D (mean), 2 D (modes), 4 (|a| + |b| + |c|) D (variance).'''
    k = X.shape[0]
    W = float(numpy.sum(w))
    sc = scales(X, w)
    m, a, b, c = numpy.asarray(coef, dtype=numpy.float64).T
    amp = numpy.abs(a) + numpy.abs(b) + numpy.abs(c)
    unit = C_BOUND * k * EPS
    rows = [('mean', mean, m, unit * sc['mean'][0] + D),
            ('variance', var, 0.5 * (a * a + b * b + c * c),
             (unit + k * EPS) * sc['M2'][0] / W + 4 * amp * D)]
    fb = 2 * (unit + k * EPS) * sc['fourier'][0] / W + 2 * D
    rows += [('re 0', f0[0], a, fb), ('im 0', f0[1], -b, fb),
             ('re 1', f1[0], c, fb), ('im 1', f1[1], 0 * c, fb)]
    for name, got, want, bound in rows:
        err = numpy.abs(numpy.asarray(got) - want)
        print('%s %s: error %.2e  bound %.2e' % (what, name, err.max(),
                                                 bound.min()))
        assert (err <= bound).all(), (what, name)
