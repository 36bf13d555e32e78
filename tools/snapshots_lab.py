# -*- coding: utf-8 -*-
'''
fem.Snapshots ("Snapshots: POD and DMD"): what the two
kernels cost, held against the box's read ceiling and against torch.

For n rows (default 8 769 868, the P2 velocity of the bench mesh) and m = 8,
16, 64 stored columns of random numbers:

  read ceiling   flow_profile_stream_read over the m = 64 store: GB/s;
  multi-dot      flow_multi_dot of m columns against one vector; the traffic
                 model 8 n (m + ceil(m / 8)) bytes over the time, as GB/s and
                 as a share of the ceiling; torch.mv on the same tensors;
  combine        flow_combine of m columns into r = 1 and r = 8 outputs;
                 8 n (m ceil(r / 8) + r) bytes; torch.matmul on the same
                 tensors.

HIP events around `batch` calls back to back, 3 warm-ups, median of 7 such
windows with min - max.  The two sides of every comparison are timed one
after the other in the same process.

  --append N     additionally: one Snapshots.append at k = 63 (copy, mass
                 product, Gram row of 64 columns) for the 2-vector P2 space on
                 UnitSquareMesh(N, N) (N = 1047: 8 778 050 rows), 'L2'.

    python tools/snapshots_lab.py [--n ROWS] [--append N]

There is no Karman demo here (a DMD Strouhal number next to one from a
lift-coefficient FFT): this tool times kernels only.
'''
import argparse
import os
import sys

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_amd import fem, device, _hip       # noqa: E402

CHUNK = 8


def timed(call, warmup=3, repeat=7, batch=10):
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


def line(what, t, nbytes, ceiling):
    gbs = nbytes / t[0] * 1e-6
    share = '' if ceiling is None else '  %5.1f %% of the read ceiling' \
        % (100.0 * gbs / ceiling)
    print('%-34s %8.4f ms (%.4f - %.4f) %8.1f GB/s%s'
          % (what, t[0], t[1], t[2], gbs, share), flush=True)


def kernels(n):
    lib = _hip.lib()
    st = _hip.stream()
    ld = n + (n & 1)
    mmax = 64
    X = torch.rand(mmax * ld, dtype=torch.float64, device=device.get()) - 0.5
    y = torch.rand(n, dtype=torch.float64, device=device.get()) - 0.5
    work = device.empty(mmax * _hip.MULTI_DOT_BLOCKS)
    sink = device.zeros(2)
    X2 = X.view(mmax, ld)[:, :n]
    t = timed(lambda: _hip.check(lib.flow_profile_stream_read(
        mmax * ld, _hip.f64(X), _hip.f64(sink), st)))
    ceiling = 8.0 * mmax * ld / t[0] * 1e-6
    print('n = %d rows' % n)
    line('read ceiling (stream read)', t, 8.0 * mmax * ld, None)
    for m in (8, 16, 64):
        out = device.empty(m)
        nbytes = 8.0 * n * (m + -(-m // CHUNK))
        t = timed(lambda: _hip.check(lib.flow_multi_dot(
            n, m, _hip.f64(X), ld, _hip.f64(y), _hip.f64(work), _hip.f64(out),
            st)))
        line('multi-dot m %2d' % m, t, nbytes, ceiling)
        Xm = X2[:m]
        tout = torch.empty(m, dtype=torch.float64, device=device.get())
        t = timed(lambda: torch.mv(Xm, y, out=tout))
        line('  torch.mv m %2d (same model)' % m, t, nbytes, ceiling)
        err = (tout - out).abs().max().item() / tout.abs().max().item()
        print('  largest difference to torch / max |out|: %.2e' % err)
        for r in (1, 8):
            C = torch.rand(r * m, dtype=torch.float64, device=device.get()) - 0.5
            res = device.empty(r * ld)
            nbytes = 8.0 * n * (m * -(-r // CHUNK) + r)
            t = timed(lambda: _hip.check(lib.flow_combine(
                n, m, _hip.f64(X), ld, r, _hip.f64(C), None, _hip.f64(res),
                ld, st)))
            line('combine m %2d r %d' % (m, r), t, nbytes, ceiling)
            C2 = C.view(r, m)
            tres = torch.empty(r, n, dtype=torch.float64, device=device.get())
            t = timed(lambda: torch.matmul(C2, Xm, out=tres))
            line('  torch.matmul m %2d r %d (same model)' % (m, r), t, nbytes,
                 ceiling)
            err = (tres - res.view(r, ld)[:, :n]).abs().max().item() \
                / tres.abs().max().item()
            print('  largest difference to torch / max |out|: %.2e' % err)
            del res, tres


def append_cost(N):
    V = fem.VectorFunctionSpace(fem.UnitSquareMesh(N, N), 'CG', 2)
    S = fem.Snapshots(V, 64, inner='L2')
    u = fem.Function(V)
    u.data.copy_(torch.rand(V.size(), dtype=torch.float64,
                            device=device.get()) - 0.5)
    for _ in range(63):
        S.append(u)

    def call():
        S._times.pop() if len(S) == 64 else None
        S.append(u)
    t = timed(call, batch=5)
    print('append at k = 63, %d rows (P2 x2 on UnitSquareMesh(%d, %d), L2): '
          '%.4f ms (%.4f - %.4f)' % (S.n, N, N, t[0], t[1], t[2]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=8769868)
    ap.add_argument('--append', type=int, default=0)
    args = ap.parse_args()
    kernels(args.n)
    if args.append:
        append_cost(args.append)


if __name__ == '__main__':
    main()
