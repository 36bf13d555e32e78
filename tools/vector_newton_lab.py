# -*- coding: utf-8 -*-
'''
Cost of one block-Newton assembly (J, F) on a vector space (DESIGN.md section
3): ops.NewtonAssembler fused (flow_form_block_newton: per row one
form_newton_kernel launch for a block and its residual component, the other
block's form_matrix_kernel launch, ONE gather for the four planes and the two
components) against fuse=False (flow_form_block_matrix +
flow_form_block_vector into held buffers) and against the baseline
assemble(J) followed by assemble(F), which allocates its results.  HIP
events around one call, 3 warm-up calls, median of 21 with min and max; the
three variants are timed in turn, twice over, and the two medians of each are
printed so that a drift of the machine shows.

    python tools/vector_newton_lab.py [nx [ny]]       (a fitted Karman channel)
'''
import os
import sys

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), 'tests'))

from flow_amd import fem, device                     # noqa: E402
from flow_amd.fem import assemble, derivative, ops   # noqa: E402


def timed(call, warmup=3, repeat=21):
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


def main():
    import vector_newton_reference as vnref
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    nx = int(args[0]) if args else 1091
    ny = int(args[1]) if len(args) > 1 else int(round(nx * 509.0 / 2182.0))
    fem.vector_arguments(True)
    fem.vector_derivatives(True)
    mesh = fem.karman_channel(nx, ny, fitted=True)
    print('mesh %d x %d: %d cells' % (nx, ny, mesh.num_cells()))
    for degree in (1, 2):
        W = fem.VectorFunctionSpace(mesh, 'CG', degree)
        print('P%d: %d dofs, %d nonzeros per block' % (degree, W.size(),
                                                      W.layout.nnz))
        for name, make in (('burgers', vnref.burgers),
                           ('forchheimer', vnref.forchheimer)):
            u = vnref.state(W)
            F = make(W, u)[0]
            J = derivative(F, u)
            fused = ops.NewtonAssembler(J, F, W)
            pair = ops.NewtonAssembler(J, F, W, fuse=False)
            assert fused.fused and not pair.fused
            variants = (('fused', fused.assemble), ('pair', pair.assemble),
                        ('assemble(J), assemble(F)',
                         lambda: (assemble(J), assemble(F))))
            med = {}
            for turn in range(2):
                for label, call in variants:
                    m, lo, hi = timed(call)
                    med.setdefault(label, []).append(m)
                    print('  P%d %-12s %-26s %.3f ms (%.3f - %.3f)'
                          % (degree, name, label, m, lo, hi))
            best = {k: min(v) for k, v in med.items()}
            print('  P%d %-12s programs %s; pair / fused = %.2f, assemble(J) + '
                  'assemble(F) / fused = %.2f'
                  % (degree, name, [len(j.program.code) for j in fused.jobs],
                     best['pair'] / best['fused'],
                     best['assemble(J), assemble(F)'] / best['fused']))


if __name__ == '__main__':
    main()
