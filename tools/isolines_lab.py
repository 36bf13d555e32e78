# -*- coding: utf-8 -*-
'''
Contour lines ("Isolines"): what fem.Isolines costs on
the bench mesh, against reading the field back and contouring it in numpy.

On the mesh of KarmanProblem(nx, ny) (default 2182 x 509: 1.1 M vertices), P1
and P2, a synthetic street -- rows of Gaussian vortices of alternating sign
behind the obstacle, as nodal values -- with 1, 8 and 32 levels spread over
its range:

  extract ms   Isolines.extract between two events on the package's stream
               (the read-back of the total sits inside); 2 warm-up calls,
               median of 7 with min - max;
  count ms     flow_isoline_count alone (one launch), the same way, and the
               share of its time that the bytes DESIGN.md names for it (the
               cell's dof indices, the unique values of f, the count) would
               take at --hbm-gbs;
  measure ms   Isolines.length (length and area come from one pass);
  numpy ms     host clock: the read-back of f, then the restatement of
               tests/isolines_reference.py on the host for the same levels
               (segments only), once.

    python tools/isolines_lab.py [--mesh NX NY] [--levels 1 8 32]
                                 [--degrees 1 2] [--repeat 7] [--no-numpy]
'''
import argparse
import ctypes
import os
import sys
import time

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from flow_amd import _hip, fem, device           # noqa: E402
from flow_amd.fem import ops                      # noqa: E402
from flow_amd.fem.isolines import _launches       # noqa: E402


def timed(call, warmup=2, repeat=7):
    '''ms per call between two events on the package's stream: median, min
    and max of `repeat` calls after `warmup`.'''
    for _ in range(warmup):
        call()
    device.synchronize()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), \
            torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return numpy.median(ms), min(ms), max(ms)


def street(xy):
    '''Two rows of Gaussian vortices of alternating sign along the channel.'''
    x, y = xy[:, 0], xy[:, 1]
    lo, hi = x.min(), x.max()
    w = numpy.zeros(len(x))
    pitch = (hi - lo) / 24.0
    for k in range(24):
        cx = lo + (k + 0.5) * pitch
        cy = 0.02 if k % 2 else -0.02
        w += (1.0 if k % 2 else -1.0) * numpy.exp(
            -((x - cx)**2 + (y - cy)**2) / (0.3 * pitch)**2)
    return w


def count_bytes(V, nc):
    '''DESIGN.md's model of the count pass: the cell's dof indices, every
    value of f once, the count.'''
    return nc * (4 * V.layout.nloc + 4) + 8 * V.N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mesh', type=int, nargs=2, default=[2182, 509])
    ap.add_argument('--levels', type=int, nargs='+', default=[1, 8, 32])
    ap.add_argument('--degrees', type=int, nargs='+', default=[1, 2])
    ap.add_argument('--repeat', type=int, default=7)
    ap.add_argument('--hbm-gbs', type=float, default=8000.0)
    ap.add_argument('--no-numpy', action='store_true')
    args = ap.parse_args()
    t0 = time.perf_counter()
    mesh = fem.karman_channel(args.mesh[0], args.mesh[1], fitted=True)
    nc = mesh.num_cells()
    print('mesh %d x %d: %d vertices, %d cells (%.1f s)'
          % (args.mesh[0], args.mesh[1], mesh.num_vertices(), nc,
             time.perf_counter() - t0), flush=True)
    lib = _hip.lib()
    for deg in args.degrees:
        V = fem.FunctionSpace(mesh, 'CG', deg)
        values = street(V.layout.dof_coords)
        f = fem.Function(V)
        f.set_array(values)
        I = fem.Isolines(V)
        mesh_s, space_s = ops.mesh_struct(mesh), ops.space_struct(V.layout)
        count = torch.empty(nc, dtype=torch.int32, device=device.get())
        print('P%d: %d dofs, %.1f MB per read-back of the field'
              % (deg, V.N, 8.0e-6 * V.N), flush=True)
        for nl in args.levels:
            levels = numpy.linspace(values.min(), values.max(), nl + 2)[1:-1]
            C = I.extract(f, levels)
            ext = timed(lambda: I.extract(f, levels), repeat=args.repeat)
            mea = timed(lambda: I.length(f, levels), repeat=args.repeat)
            L = _launches(levels)[0]

            def count_once():
                _hip.check(lib.flow_isoline_count(
                    ctypes.byref(mesh_s), ctypes.byref(space_s),
                    _hip.f64(f.data, V.N), ctypes.byref(L),
                    _hip.i32(count, nc), _hip.stream()))

            cnt = timed(count_once, repeat=args.repeat)
            ideal = count_bytes(V, nc) / (args.hbm_gbs * 1.0e6)      # ms
            line = ('    %2d levels: %8d segments, extract %7.3f ms (%.3f - '
                    '%.3f), count %6.3f ms = %5.1f GB/s (%4.1f %% of %g), '
                    'measure %7.3f ms'
                    % (nl, C.nseg, ext[0], ext[1], ext[2], cnt[0],
                       count_bytes(V, nc) / cnt[0] * 1.0e-6,
                       100.0 * ideal / cnt[0], args.hbm_gbs, mea[0]))
            if not args.no_numpy:
                import isolines_reference as iref
                t0 = time.perf_counter()
                back = f.array()
                t1 = time.perf_counter()
                s = iref.segments(V.layout, back, levels)
                t2 = time.perf_counter()
                assert len(s['cell']) == C.nseg
                line += (', numpy %.0f ms (read-back %.1f ms)'
                         % (1.0e3 * (t2 - t0), 1.0e3 * (t1 - t0)))
            print(line, flush=True)


if __name__ == '__main__':
    main()
