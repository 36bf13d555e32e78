# -*- coding: utf-8 -*-
'''
Cost of fem.Supermesh ("Norms across meshes"): a P2
vector field on the fitted channel karman_channel(nx, ny) -- the bench mesh
at the default size -- against its interpolant on a once-refined copy
(fem.refine, every cell), and back.

  construction  Supermesh(...): pair list, upload, the geometry launch, the
                read-back of the coverage (wall clock: it synchronises);
  cell_errors   flow_supermesh_norms: the one launch, both planes;
  errornorm     the same, the two fixed-order sums and their read-back;
  load          Projection.load between the same spaces: the same clips with
                the load vector's integrand, and its gather.

HIP events, 2 warm-up calls, median of 7 with min and max.

    python tools/supermesh_norm_lab.py [nx [ny]]
'''
import os
import sys
import time

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_amd import fem, device       # noqa: E402


def timed(call, warmup=2, repeat=7):
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


def one_way(what, u, w):
    V_a, V_b = u.function_space(), w.function_space()
    device.synchronize()
    t0 = time.perf_counter()
    S = fem.Supermesh(V_a, V_b, allow_partial=True)
    device.synchronize()
    t1 = time.perf_counter()
    print('%s: %d -> %d cells, %d pairs; construction %.3f s wall; min '
          'coverage %.15f; area %.12f'
          % (what, V_a.mesh().num_cells(), V_b.mesh().num_cells(), S.pairs,
             t1 - t0, S.min_coverage, S.area))
    print('  |u - w|: L2 %.6e  H10 %.6e  (|u|_L2 %.6e)'
          % (S.errornorm(u, w), S.errornorm(u, w, 'H10'), fem.norm(u)))
    print('  cell_errors          %9.3f ms (%.3f - %.3f)'
          % timed(lambda: S.cell_errors(u, w)))
    print('  errornorm            %9.3f ms (%.3f - %.3f)'
          % timed(lambda: S.errornorm(u, w)))
    P = fem.Projection(V_a, V_b, allow_partial=True)
    print('  Projection.load      %9.3f ms (%.3f - %.3f)'
          % timed(lambda: P.load(u)))


def main():
    args = sys.argv[1:]
    nx = int(args[0]) if args else 2182
    ny = int(args[1]) if len(args) > 1 else int(round(nx * 509.0 / 2182.0))
    coarse = fem.karman_channel(nx, ny, fitted=True)
    fine = fem.refine(coarse)
    V_c = fem.VectorFunctionSpace(coarse, 'CG', 2)
    V_f = fem.VectorFunctionSpace(fine, 'CG', 2)
    field = fem.Expression(('sin(20*x[0])*x[1] + 1.0',
                            'cos(15*x[1])*x[0] - 0.5'), degree=2)
    u_c = fem.interpolate(field, V_c)
    u_f = fem.interpolate(field, V_f)
    one_way('coarse -> fine', u_c, u_f)
    one_way('fine -> coarse', u_f, u_c)


if __name__ == '__main__':
    main()
