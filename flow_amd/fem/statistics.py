# -*- coding: utf-8 -*-
'''
Running time statistics of a field, accumulated on the GPU while the solver
runs: time-averaged fields and their RMS, Reynolds stresses, peak values with
the times they occurred at, and the spatial Fourier modes at chosen
frequencies, over a run of any length (nothing but the accumulators is kept).

    S = Statistics(V, covariance=True, frequencies=(), extrema=False)
    S.update(u, dt=1.0, t=None)     # one sample with weight dt > 0, taken at t
    S.weight; S.count; S.t_first; S.t_last   # host numbers, no read-back
    S.mean(out=None)                # Function on V
    S.variance(out=None); S.rms(out=None)    # Function on V, per component,
                                    # population (weight-normalised)
    S.covariance()                  # scalar V: (var,); 2-vector V: (uu, uv, vv)
    S.tke(out=None)                 # 2-vector V only: (uu + vv) / 2
    S.fourier(k)                    # (re, im) Functions on V for frequencies[k]
    S.minimum(); S.maximum(); S.time_of_minimum(); S.time_of_maximum()
    S.merge(other)                  # S becomes the statistics of both sample sets
    S.reset()
    S.state(); Statistics.from_state(V, state)   # numpy arrays, host scalars

V is a scalar or 2-vector P1 / P2 space.  `frequencies`: at most
FLOW_STATS_MAX_FREQ = 8 positive numbers in 1 / (unit of t); with frequencies
or with extrema=True every update needs its t.

The store is one device tensor of planes of ld doubles each, ld = V.N rounded
up to even (every plane 16-byte aligned), in this order: mean[dim], M2[1 or 3]
(covariance), per frequency A_k[dim], B_k[dim], then min, max, tmin, tmax [dim
each] (extrema).  Padding entries are never read for a result and never
written.

Definitions (flow_stats_update, csrc/stats_kernels.hip).  Per dof i and
component a, with host scalars W' = W + w, r = w / W', s = w * W / W':

    delta_a = x_a - mean_a
    mean_a  = fma(r, delta_a, mean_a)
    M2_ab   = fma(s * delta_a, delta_b, M2_ab)        (ab = 00; or 00, 01, 11)
    A_k,a   = fma(w cos phi_k, x_a, A_k,a)
    B_k,a   = fma(-w sin phi_k, x_a, B_k,a)     phi_k = 2 pi * fmod(f_k * t, 1)
    if x_a < min_a: min_a = x_a, tmin_a = t      (strict: the first occurrence
                                                  stays; likewise max)

The first update has W = 0, so r = 1 and s = 0: mean == x bit for bit (but
for the sign of a zero: -0.0 + 0.0 is +0.0) and M2 == 0.0; a constant field
keeps M2 == 0.0 exactly.  A diagonal M2 never goes
below zero, so variance() is never negative and rms() never NaN.  fourier(k)
is (2 / W) (A_k, B_k): a field m + a cos(2 pi f t) + b sin(2 pi f t) sampled
over whole periods gives re = a, im = -b, that is u ~ mean + Re((re + i im)
exp(2 pi i f t)).  The cos and sin are taken on the host.  NaN in x makes the
moments NaN; the comparisons of the extrema are false for NaN (a dof that was
never below +inf keeps min = +inf and the time NaN).

update() is ONE kernel launch: r, s, t and the up to 8 coefficient pairs
travel as kernel arguments, nothing is uploaded and the device is never waited
for.  The getters are a cold path: copies and scalings by flow_axpby, the
square root by torch, on the package's stream.

merge(other) is Chan's combination (flow_stats_merge), W = Wa + Wb:

    d = mean_b - mean_a
    mean = fma(Wb / W, d, mean_a)
    M2_ab = fma((Wa Wb / W) d_a, d_b, M2a_ab + M2b_ab)
    A, B add
    extrema by comparison, the time taken from the winner (ties keep self's)

Merging an empty `other` launches nothing; merging into an empty self copies.

state() synchronises and reads the planes back; from_state checks shapes and
options.  Not on strips.
'''
import ctypes
import math

import numpy

MAX_FREQ = 8                    # FLOW_STATS_MAX_FREQ (include/flow_hip.h)


# -- host scalars (plain Python floats: IEEE double, one rounding per operation) -----
def update_scalars(W, w):
    '''(W', r, s) of an update with weight w behind the weight W.'''
    W1 = W + w
    return W1, w / W1, (w * W) / W1


def merge_scalars(Wa, Wb):
    '''(W, q, g) of a merge of the weights Wa and Wb (W > 0).'''
    W = Wa + Wb
    return W, Wb / W, (Wa * Wb) / W


def fourier_coefficients(frequencies, w, t):
    '''[(w cos phi_k, -w sin phi_k)], phi_k = 2 pi fmod(f_k t, 1).'''
    out = []
    for f in frequencies:
        phi = (2.0 * math.pi) * math.fmod(f * t, 1.0)
        out.append((w * math.cos(phi), -(w * math.sin(phi))))
    return out


def plane_layout(dim, covariance, nfreq, extrema):
    '''{name: first plane} and the number of planes of a store.'''
    at = {'mean': 0}
    p = dim
    if covariance:
        at['M2'] = p
        p += 1 if dim == 1 else 3
    at['fourier'] = p
    p += 2 * dim * nfreq
    if extrema:
        for name in ('min', 'max', 'tmin', 'tmax'):
            at[name] = p
            p += dim
    return at, p


# -- the space ----------------------------------------------------------------------
def _no_strips():
    from .. import parallel
    if parallel.active():
        raise NotImplementedError(
            'Statistics on strips is not implemented: a rank holds its own '
            'rows only')


def _check_space(V):
    if not hasattr(V, 'layout'):
        raise NotImplementedError(
            'V: a mixed space; keep the statistics of its sub-spaces one by '
            'one')
    if getattr(V, 'component', None) is not None:
        raise NotImplementedError(
            'V: a component view (W.sub(i)); keep the statistics of the '
            'vector field, or of Functions on W.sub(i).collapse()')
    if V.degree not in (1, 2):
        raise ValueError('V: P%r; statistics take P1 or P2' % (V.degree,))
    if V.dim not in (1, 2):
        raise ValueError('V: %r components; scalar or 2-vector' % (V.dim,))
    _no_strips()


def _check_frequencies(frequencies):
    fs = tuple(float(f) for f in frequencies)
    if len(fs) > MAX_FREQ:
        raise ValueError('frequencies: %d of them; at most %d'
                         % (len(fs), MAX_FREQ))
    if not all(f > 0.0 and math.isfinite(f) for f in fs):
        raise ValueError('frequencies: positive numbers')
    return fs


class Statistics(object):
    '''Weighted running mean, second moments, Fourier sums and extrema of
    Functions of V (scalar or 2-vector P1 / P2); see the module's text.'''

    def __init__(self, V, covariance=True, frequencies=(), extrema=False):
        from .. import device
        from .space import FunctionSpace
        _check_space(V)
        self.V = V
        self.covariance_kept = bool(covariance)
        self.frequencies = _check_frequencies(frequencies)
        self.extrema = bool(extrema)
        self.N = V.N
        self.ld = self.N + (self.N & 1)
        self._at, self.planes = plane_layout(
            V.dim, self.covariance_kept, len(self.frequencies), self.extrema)
        self._flags = (1 if self.covariance_kept else 0) \
            | (2 if self.extrema else 0)
        # the space of the per-component results (covariance, tke)
        self.scalar_space = V if V.dim == 1 else \
            FunctionSpace(V.mesh(), 'CG', V.degree)
        self._P = device.empty(self.planes * self.ld)
        self.reset()

    # -- bookkeeping ---------------------------------------------------------------
    def reset(self):
        '''Forget every sample (the store and the options stay).'''
        from .. import _hip
        self.weight, self.count = 0.0, 0
        self.t_first = self.t_last = None
        ld = self.ld
        first = self._at.get('min', self.planes)
        if self._P.numel() > 0:
            _hip.fill(self._P[:first * ld], 0.0)
        if self.extrema and self._P.numel() > 0:
            dim = self.V.dim
            lo, hi, tt = self._at['min'], self._at['max'], self._at['tmin']
            _hip.fill(self._P[lo * ld:(lo + dim) * ld], float('inf'))
            _hip.fill(self._P[hi * ld:(hi + dim) * ld], float('-inf'))
            _hip.fill(self._P[tt * ld:(tt + 2 * dim) * ld], float('nan'))

    def _needs_t(self):
        return bool(self.frequencies) or self.extrema

    def _check_u(self, u, what='u'):
        from .function import Function
        if not isinstance(u, Function) \
                or not u.function_space().same_as(self.V):
            raise ValueError('%s: not a Function of the space these '
                             'statistics were built for' % what)

    def _plane(self, p):
        return self._P[p * self.ld:p * self.ld + self.N]

    # -- accumulation -----------------------------------------------------------------
    def update(self, u, dt=1.0, t=None):
        '''One sample: the Function u with weight dt > 0, taken at time t
        (needed with frequencies or extrema).  One kernel launch on the
        package's stream; no upload, no synchronisation.'''
        from .. import _hip
        _no_strips()
        self._check_u(u)
        w = float(dt)
        if not (w > 0.0 and math.isfinite(w)):
            raise ValueError('dt: a positive weight')
        if t is None:
            if self._needs_t():
                raise ValueError('t: statistics with frequencies or extrema '
                                 'need the time of every sample')
            tt = 0.0
        else:
            tt = float(t)
            if not math.isfinite(tt):
                raise ValueError('t: a finite time')
        lib = _hip.lib()
        W1, r, s = update_scalars(self.weight, w)
        freq = _hip.StatsFreq()
        freq.n = len(self.frequencies)
        for k, (c, sn) in enumerate(
                fourier_coefficients(self.frequencies, w, tt)):
            freq.c[k], freq.s[k] = c, sn
        dim = self.V.dim
        _hip.check(lib.flow_stats_update(
            self.N, dim, self._flags, ctypes.byref(freq), r, s, tt,
            _hip.f64(u.data, dim * self.N, 'u'),
            _hip.f64(self._P, self.planes * self.ld, 'planes'), self.ld,
            _hip.stream()))
        self.weight = W1
        self.count += 1
        if t is not None:
            if self.t_first is None:
                self.t_first = tt
            self.t_last = tt

    def _same_options(self, other):
        return (isinstance(other, Statistics) and other.V.same_as(self.V)
                and other.covariance_kept == self.covariance_kept
                and other.extrema == self.extrema
                and other.frequencies == self.frequencies)

    def merge(self, other):
        '''Combine with the statistics `other` of another set of samples of
        the same space, options and frequencies: self becomes the statistics
        of both sets (other is left as it is).'''
        from .. import _hip
        _no_strips()
        if other is self or not self._same_options(other):
            raise ValueError('other: Statistics of the same space, options '
                             'and frequencies (and not self)')
        if other.weight == 0.0:
            return
        if self.weight == 0.0:
            _hip.lib()
            _hip.copy(self._P, other._P)
        else:
            W, q, g = merge_scalars(self.weight, other.weight)
            _hip.check(_hip.lib().flow_stats_merge(
                self.N, self.V.dim, self._flags, len(self.frequencies), q, g,
                _hip.f64(self._P, self.planes * self.ld, 'planes'),
                _hip.f64(other._P, self.planes * self.ld, 'other'), self.ld,
                _hip.stream()))
        self.weight = self.weight + other.weight
        self.count += other.count
        firsts = [s.t_first for s in (self, other) if s.t_first is not None]
        lasts = [s.t_last for s in (self, other) if s.t_last is not None]
        self.t_first = min(firsts) if firsts else None
        self.t_last = max(lasts) if lasts else None

    # -- results (a cold path) ---------------------------------------------------------
    def _ready(self, need=None):
        if need == 'covariance' and not self.covariance_kept:
            raise ValueError('built with covariance=False: no second moments')
        if need == 'extrema' and not self.extrema:
            raise ValueError('built with extrema=False')
        if self.weight == 0.0:
            raise ValueError('no samples')

    def _out(self, out, V=None):
        from .function import Function
        V = self.V if V is None else V
        if out is None:
            return Function(V)
        if not isinstance(out, Function) or not out.function_space().same_as(V) \
                or getattr(out.function_space(), 'component', None) is not None:
            raise ValueError('out: not a Function of the space of this result')
        return out

    def _scaled(self, a, plane, dst):
        '''dst = a * plane (tensors of N doubles).'''
        from .. import _hip
        _hip.check(_hip.lib().flow_axpby(
            self.N, float(a), _hip.f64(plane, self.N, 'plane'), 0.0,
            _hip.f64(dst, self.N, 'out'), _hip.stream()))

    def _vector(self, first, a, out):
        '''a * planes first..first+dim as a Function of V.'''
        out = self._out(out)
        N = self.N
        for c in range(self.V.dim):
            self._scaled(a, self._plane(first + c), out.data[c * N:(c + 1) * N])
        return out

    def mean(self, out=None):
        self._ready()
        return self._vector(self._at['mean'], 1.0, out)

    def _diagonal(self, c):
        return self._at['M2'] + (0 if c == 0 else 2)

    def variance(self, out=None):
        '''M2_aa / W per component, a Function of V.'''
        self._ready('covariance')
        out = self._out(out)
        N = self.N
        for c in range(self.V.dim):
            self._scaled(1.0 / self.weight, self._plane(self._diagonal(c)),
                         out.data[c * N:(c + 1) * N])
        return out

    def rms(self, out=None):
        '''sqrt(variance) per component, a Function of V.'''
        import torch
        out = self.variance(out)
        torch.sqrt(out.data, out=out.data)
        return out

    def covariance(self):
        '''(var,) for a scalar V, (uu, uv, vv) for a 2-vector V: Functions of
        `scalar_space`.'''
        self._ready('covariance')
        fs = []
        for p in range(1 if self.V.dim == 1 else 3):
            f = self._out(None, self.scalar_space)
            self._scaled(1.0 / self.weight, self._plane(self._at['M2'] + p),
                         f.data)
            fs.append(f)
        return tuple(fs)

    def tke(self, out=None):
        '''(uu + vv) / 2 of a 2-vector V, a Function of `scalar_space`.'''
        from .. import _hip
        if self.V.dim != 2:
            raise ValueError('tke: of a 2-vector field')
        self._ready('covariance')
        out = self._out(out, self.scalar_space)
        a = 0.5 / self.weight
        self._scaled(a, self._plane(self._diagonal(0)), out.data)
        _hip.check(_hip.lib().flow_axpby(
            self.N, a, _hip.f64(self._plane(self._diagonal(1)), self.N, 'vv'),
            1.0, _hip.f64(out.data, self.N, 'out'), _hip.stream()))
        return out

    def fourier(self, k):
        '''(re, im) = (2 / W) (A_k, B_k), Functions of V.'''
        if not 0 <= k < len(self.frequencies):
            raise IndexError('frequency %r of %d' % (k, len(self.frequencies)))
        self._ready()
        dim = self.V.dim
        first = self._at['fourier'] + 2 * dim * k
        a = 2.0 / self.weight
        return self._vector(first, a, None), self._vector(first + dim, a, None)

    def minimum(self):
        self._ready('extrema')
        return self._vector(self._at['min'], 1.0, None)

    def maximum(self):
        self._ready('extrema')
        return self._vector(self._at['max'], 1.0, None)

    def time_of_minimum(self):
        self._ready('extrema')
        return self._vector(self._at['tmin'], 1.0, None)

    def time_of_maximum(self):
        self._ready('extrema')
        return self._vector(self._at['tmax'], 1.0, None)

    # -- state transfer -----------------------------------------------------------------
    def state(self):
        '''A dict of numpy arrays and host scalars that from_state turns back
        into an equal object; synchronises and reads the planes back.'''
        from .. import device
        planes = device.to_host(self._P).numpy().reshape(
            self.planes, self.ld)[:, :self.N].copy()
        return {
            'planes': planes, 'weight': self.weight, 'count': self.count,
            't_first': self.t_first, 't_last': self.t_last,
            'dim': self.V.dim, 'degree': self.V.degree, 'N': self.N,
            'covariance': self.covariance_kept, 'extrema': self.extrema,
            'frequencies': numpy.array(self.frequencies, dtype=float),
            }

    @classmethod
    def from_state(cls, V, state):
        '''The Statistics on V that state() was taken from.'''
        from .. import device
        try:
            planes = numpy.asarray(state['planes'], dtype=numpy.float64)
            S = cls(V, covariance=bool(state['covariance']),
                    frequencies=tuple(numpy.asarray(
                        state['frequencies'], dtype=float).reshape(-1)),
                    extrema=bool(state['extrema']))
            same = (int(state['dim']) == V.dim
                    and int(state['degree']) == V.degree
                    and int(state['N']) == V.N)
            weight, count = float(state['weight']), int(state['count'])
            t_first, t_last = state['t_first'], state['t_last']
        except KeyError as e:
            raise ValueError('state: no entry %s' % e)
        if not same or planes.shape != (S.planes, S.N):
            raise ValueError('state: taken from another space or other '
                             'options (planes %r, here %r)'
                             % (planes.shape, (S.planes, S.N)))
        if not (weight >= 0.0 and count >= 0):
            raise ValueError('state: weight and count')
        full = numpy.zeros((S.planes, S.ld))
        full[:, :S.N] = planes
        S._P.copy_(device.to_device(full.reshape(-1)))
        device.synchronize()
        S.weight, S.count = weight, count
        S.t_first = None if t_first is None else float(t_first)
        S.t_last = None if t_last is None else float(t_last)
        return S
