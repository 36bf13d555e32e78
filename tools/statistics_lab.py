# -*- coding: utf-8 -*-
'''
fem.Statistics ("Running statistics"): what one update
costs on the bench mesh, held against the same update spelled with torch
operations and against the bytes it has to move.

The space is the P2 velocity of the bench mesh, karman_channel(2182, 509,
fitted=True) (what KarmanProblem(2182, 509) builds; the problem's boundary
conditions and steppers are not needed here).  For the option sets

    mean | mean + covariance | + 2 frequencies | + extrema

it times one Statistics.update (one launch of flow_stats_update) on a field of
random numbers, and the same update as a composition of torch operations on
views of a copy of the same store (sub, add, addcmul, where: one pass over the
operands per operation).  HIP events around `batch` calls back to back, 2
warm-ups, median of 7 such windows with min - max; the two sides are timed one
after the other in the same process.  The byte count is the kernel header's,
8 N dim + 16 N planes; "at 5.8 TB/s" is that count over the rate README.md
quotes for a streaming kernel on this box.  Nothing is asserted.

    python tools/statistics_lab.py [--nx 2182] [--ny 509] [--batch 5]
'''
import argparse
import os
import sys

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_amd import fem, device       # noqa: E402
from flow_amd.fem import statistics    # noqa: E402

STREAM_RATE = 5.8e12        # B/s, README.md


def timed(call, warmup=2, repeat=7, batch=5):
    '''ms per call: median, min and max of `repeat` windows of `batch` calls
    between two events.'''
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


def torch_update(S, P, x, w, t):
    '''The update of S's definitions on the store P (a tensor laid out as
    S._P) with torch operations, one per line of the definitions.'''
    dim, N, ld, at = S.V.dim, S.N, S.ld, S._at

    def plane(p):
        return P[p * ld:p * ld + N]
    W1, r, s = statistics.update_scalars(S.weight, w)
    xs = [x[a * N:(a + 1) * N] for a in range(dim)]
    d = []
    for a in range(dim):
        m = plane(at['mean'] + a)
        d.append(xs[a] - m)
        m.add_(d[a], alpha=r)
    if S.covariance_kept:
        p = at['M2']
        for a in range(dim):
            for b in range(a, dim):
                plane(p).addcmul_(d[a], d[b], value=s)
                p += 1
    p = at['fourier']
    for c, sn in statistics.fourier_coefficients(S.frequencies, w, t):
        for a in range(dim):
            plane(p + a).add_(xs[a], alpha=c)
            plane(p + dim + a).add_(xs[a], alpha=sn)
        p += 2 * dim
    if S.extrema:
        for a in range(dim):
            for key, tkey, op in (('min', 'tmin', torch.lt),
                                  ('max', 'tmax', torch.gt)):
                v, tv = plane(at[key] + a), plane(at[tkey] + a)
                hit = op(xs[a], v)
                torch.where(hit, xs[a], v, out=v)
                tv.masked_fill_(hit, t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=2182)
    ap.add_argument('--ny', type=int, default=509)
    ap.add_argument('--batch', type=int, default=5)
    args = ap.parse_args()
    mesh = fem.karman_channel(args.nx, args.ny, fitted=True)
    V = fem.VectorFunctionSpace(mesh, 'CG', 2)
    u = fem.Function(V)
    u.data.copy_(torch.rand(V.size(), dtype=torch.float64,
                            device=device.get()) - 0.5)
    print('P2 velocity on karman_channel(%d, %d): N = %d, %d DoF'
          % (args.nx, args.ny, V.N, V.size()), flush=True)
    print('%-28s %6s %9s  %-30s %-30s %7s %9s %9s' % (
        'options', 'planes', 'MB', 'update, ms (min - max)',
        'torch, ms (min - max)', 'torch/', 'GB/s', 'of 5.8'))
    sets = [('mean', dict(covariance=False)),
            ('mean + covariance', dict(covariance=True)),
            ('+ 2 frequencies', dict(covariance=True, frequencies=(3.0, 6.0))),
            ('+ extrema', dict(covariance=True, frequencies=(3.0, 6.0),
                               extrema=True))]
    w, t = 1.0e-3, 0.123
    for name, opts in sets:
        S = fem.Statistics(V, **opts)
        S.update(u, dt=w, t=t)                 # W > 0: the general r and s
        nbytes = 8.0 * V.N * V.dim + 16.0 * V.N * S.planes
        P = S._P.clone()
        # one update on each side from the same state: how far apart?
        weight = S.weight
        torch_update(S, P, u.data, w, t)
        S.update(u, dt=w, t=t)
        S.weight, S.count = weight, S.count - 1
        diff = (S._P - P).view(S.planes, S.ld)[:, :S.N].abs().max().item()
        ours = timed(lambda: (S.update(u, dt=w, t=t),
                              setattr(S, 'weight', weight)), batch=args.batch)
        theirs = timed(lambda: torch_update(S, P, u.data, w, t),
                       batch=args.batch)
        gbs = nbytes / ours[0] * 1e-6
        print('%-28s %6d %9.1f  %-30s %-30s %7.2f %9.1f %8.1f%%   '
              '(model at 5.8 TB/s: %.4f ms; largest difference to torch %.1e)'
              % (name, S.planes, nbytes * 1e-6,
                 '%.4f (%.4f - %.4f)' % ours, '%.4f (%.4f - %.4f)' % theirs,
                 theirs[0] / ours[0], gbs, 100.0 * gbs * 1e9 / STREAM_RATE,
                 nbytes / STREAM_RATE * 1e3, diff), flush=True)
        del S, P


if __name__ == '__main__':
    main()
