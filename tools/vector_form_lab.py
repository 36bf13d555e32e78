# -*- coding: utf-8 -*-
'''
Cost of forms of arguments on a vector space, flow_form_block_matrix (one
element launch per program, ONE four-plane gather), on the bench mesh
("Arguments on vector spaces"): HIP events, 2 warm-up
calls, median of 7 with min and max, structs built once outside the timed
call.  Rows: the vector Laplacian, the vector mass matrix and the elasticity
operator, P1 and P2.  The yardstick of a row is the scalar path on the same
programs: flow_form_matrix (element launch + one-plane gather) once per
present block, each into the block's plane -- which is also what "one gather
per block" would cost.  That path leaves the planes of absent blocks alone;
flow_form_block_matrix writes them as zeros, so a third column adds the fill
of the absent planes to the yardstick: what a caller of the scalar path
pays for the same result.

    python tools/vector_form_lab.py [nx [ny]]
'''
import ctypes
import os
import sys

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_amd import fem, device, _hip               # noqa: E402
from flow_amd.fem import (                           # noqa: E402
    TestFunction, TrialFunction, dx, dot, inner, grad, sym, tr, Identity,
    forms, ops,
    )


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


def calls(form):
    '''(block call, per-block scalar calls, present blocks) of a one-part
    rank-2 form on a vector space.'''
    lib = _hip.lib()
    W = form.arguments()[0]
    lay, mesh = W.layout, W.mesh()
    nc = mesh.num_cells()
    (_, part), = form.terms()
    _, table = part.argument_table()
    progs = [(p, prog) for p, block in forms.block_items(table, 2)
             for prog in forms.argument_programs(block, 2)]
    jobs = [ops._form_struct(prog, mesh, part.degree()) for _, prog in progs]
    structs = (_hip.FormS * len(progs))()
    for k, (fs, _) in enumerate(jobs):
        structs[k] = fs
    tags = (ctypes.c_int * len(progs))(*[p for p, _ in progs])
    present = len(set(p for p, _ in progs))
    plane = lay.nloc**2 * nc
    ns = (present + (len(progs) > present)) * plane
    buf = ops.scratch(mesh, ns)
    stride = ops.plane_stride(lay)
    out = device.zeros(4 * stride)
    ms, ss = ops.mesh_struct(mesh), ops.space_struct(lay)

    def block():
        _hip.check(lib.flow_form_block_matrix(
            ctypes.byref(ms), ctypes.byref(ss), len(progs), structs, tags,
            _hip.f64(buf, ns, 'scratch'), _hip.f64(out, 4 * stride, 'vals'),
            stride, _hip.stream()))

    def scalar():
        for (p, _), (fs, _) in zip(progs, jobs):
            _hip.check(lib.flow_form_matrix(
                ctypes.byref(ms), ctypes.byref(ss), ctypes.byref(fs),
                _hip.f64(buf, plane, 'scratch'),
                _hip.f64(out[p * stride:p * stride + lay.nnz], lay.nnz,
                         'vals'), _hip.stream()))
    absent = [p for p in range(4) if p not in set(q for q, _ in progs)]

    def scalar_zeroed():
        scalar()
        for p in absent:
            _hip.fill(out[p * stride:p * stride + lay.nnz], 0.0)
    return block, scalar, scalar_zeroed, present, len(progs)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    nx = int(args[0]) if args else 2182
    ny = int(args[1]) if len(args) > 1 else int(round(nx * 509.0 / 2182.0))
    mesh = fem.karman_channel(nx, ny, fitted=True)
    print('mesh %d x %d: %d cells' % (nx, ny, mesh.num_cells()))
    mu, lam = fem.Constant(1.0), fem.Constant(1.5)

    def eps(w):
        return sym(grad(w))

    with fem.vector_arguments(True):
        for degree in (1, 2):
            W = fem.VectorFunctionSpace(mesh, 'CG', degree)
            u, v = TrialFunction(W), TestFunction(W)
            for name, a in (
                    ('vector Laplacian', inner(grad(u), grad(v)) * dx),
                    ('vector mass', dot(u, v) * dx),
                    ('elasticity', inner(2.0 * mu * eps(u) + lam * tr(eps(u))
                                         * Identity(2), eps(v)) * dx)):
                block, scalar, zeroed, present, nprog = calls(a)
                tb = timed(block)
                ts = timed(scalar)
                tz = timed(zeroed)
                print('P%d %-17s %d blocks, %d programs: block %.3f ms (%.3f '
                      '- %.3f), scalar path per block %.3f ms (%.3f - %.3f), '
                      'ratio %.2f; with the absent planes filled %.3f ms '
                      '(%.3f - %.3f), ratio %.2f'
                      % ((degree, name, present, nprog) + tuple(tb)
                         + tuple(ts) + (tb[0] / ts[0],) + tuple(tz)
                         + (tb[0] / tz[0],)))


if __name__ == '__main__':
    main()
