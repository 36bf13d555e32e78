# -*- coding: utf-8 -*-
'''
Cost of the generic matrix path, flow_form_matrix, against the dedicated
kernels on the bench mesh ("Cost of the generic path"):
kernel + gather through the C entry point with a prebuilt flow_form, HIP
events, 2 warm-up calls, median of 7 with min and max.  Rows: P1 stiffness,
P2 mass, P2 heat operator without SUPG; where the tree has them, the P1 SUPG
heat operator from the reference's form text (its parts, one launch each;
the tau lattice is built once, outside the timed call, and timed on its own
line) against flow_assemble_heat with SUPG, and flow_supg_tau against the
tau-by-assembly it replaces.  The first three rows run on any commit that
has forms of arguments: to judge a change of the interpreter, run the script
on the change and on its parent, same machine, same session.

    python tools/form_cost_lab.py [nx [ny]]
'''
import ctypes
import os
import sys

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_amd import fem, device, _hip               # noqa: E402
from flow_amd.fem import (                           # noqa: E402
    TestFunction, TrialFunction, dx, dot, inner, grad, forms, ops,
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


def generic(form):
    '''A call that runs flow_form_matrix for every program of every part of
    the rank-2 form (kernel + gather each; structs built once).'''
    lib = _hip.lib()
    V = form.arguments()[0]
    lay, mesh = V.layout, V.mesh()
    nc = mesh.num_cells()
    jobs = []
    for sign, part in form.terms():
        _, table = part.argument_table()
        for prog in forms.argument_programs(table, 2):
            jobs.append(ops._form_struct(prog, mesh, part.degree()))
    out = ops.value_plane(lay)
    buf = ops.scratch(mesh, lay.nloc**2 * nc)
    ms, ss = ops.mesh_struct(mesh), ops.space_struct(lay)

    def call():
        for fs, keep in jobs:
            _hip.check(lib.flow_form_matrix(
                ctypes.byref(ms), ctypes.byref(ss), ctypes.byref(fs),
                _hip.f64(buf, lay.nloc**2 * nc, 'scratch'),
                _hip.f64(out, lay.nnz, 'vals'), _hip.stream()))
    return call, len(jobs)


def heat(V, conv, kappa, rho_cp, supg):
    lib = _hip.lib()
    lay, mesh = V.layout, V.mesh()
    W = conv.function_space()
    nc = mesh.num_cells()
    A = ops.value_plane(lay)
    Ms = ops.value_plane(lay)
    tau = device.empty(3 * nc)
    status = device.zeros(1, dtype=torch.int32)
    buf = ops.scratch(mesh, 2 * lay.nloc**2 * nc)
    ms, qs, ws = ops.mesh_struct(mesh), ops.space_struct(lay), \
        ops.space_struct(W.layout)

    def call():
        _hip.check(lib.flow_assemble_heat(
            ctypes.byref(ms), ctypes.byref(qs), ctypes.byref(ws),
            _hip.f64(conv.data, W.size()), kappa, rho_cp, int(supg),
            _hip.f64(buf), _hip.f64(A), _hip.f64(Ms), _hip.f64(tau),
            _hip.i32(status), _hip.stream()))
    return call


def row(name, t):
    print('%-44s %.3f ms (%.3f - %.3f)' % ((name,) + tuple(t)))
    return t


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    nx = int(args[0]) if args else 2182
    ny = int(args[1]) if len(args) > 1 else int(round(nx * 509.0 / 2182.0))
    lib = _hip.lib()
    mesh = fem.karman_channel(nx, ny, fitted=True)
    nc = mesh.num_cells()
    print('mesh %d x %d: %d cells' % (nx, ny, nc))
    V1 = fem.FunctionSpace(mesh, 'CG', 1)
    V2 = fem.FunctionSpace(mesh, 'CG', 2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    conv = fem.Function(W)
    xy = W.layout.dof_coords
    conv.set_array(numpy.concatenate([1.0 + xy[:, 0] * xy[:, 1] - xy[:, 1]**2,
                                      0.5 * xy[:, 0]**2 - xy[:, 1]]))
    kappa, rho_cp = 0.37, 1.3 * 2.1
    kap = fem.Constant(kappa)

    u, v = TrialFunction(V1), TestFunction(V1)
    call, _ = generic(inner(grad(u), grad(v)) * dx)
    row('P1 stiffness, generic', timed(call))
    row('P1 stiffness, dedicated', timed(
        lambda: ops.assemble_scalar_matrix(V1.layout, ops.STIFFNESS)))

    u, v = TrialFunction(V2), TestFunction(V2)
    call, _ = generic(u * v * dx)
    row('P2 mass, generic', timed(call))
    row('P2 mass, dedicated', timed(
        lambda: ops.assemble_scalar_matrix(V2.layout, ops.MASS)))
    F = - kap * dot(grad(u), grad(v / rho_cp)) * dx \
        - dot(conv, grad(u)) * v * dx
    call, n = generic(forms.lhs(F))
    row('P2 heat operator (no SUPG), generic, %d launches' % n, timed(call))
    row('P2 heat operator (no SUPG), dedicated',
        timed(heat(V2, conv, kappa, rho_cp, False)))

    if not hasattr(forms, 'conditional'):
        return
    from flow_amd import stabilization
    u, v = TrialFunction(V1), TestFunction(V1)
    tau = stabilization.supg(mesh, conv, kappa, 1)
    F = - kap * dot(grad(u), grad(v / rho_cp)) * dx \
        - dot(conv, grad(u)) * v * dx \
        + (- dot(conv, grad(u))) * tau * dot(conv, grad(v)) * dx \
        + u * tau * dot(conv, grad(v)) * dx
    call, n = generic(F)
    row('P1 SUPG heat operator (A and M supg), generic, %d launches' % n,
        timed(call))
    row('P1 SUPG heat operator (A and M supg), dedicated',
        timed(heat(V1, conv, kappa, rho_cp, True)))
    row('tau by assembly (cell_vertex_values, host copy included)',
        timed(tau.cell_vertex_values))
    row('tau by flow_supg_tau (form_lattice: status read included)',
        timed(lambda: tau.form_lattice(mesh)))
    for p in (1, 2):
        status = device.zeros(1, dtype=torch.int32)
        out = device.empty(3 * nc)
        ms, ws = ops.mesh_struct(mesh), ops.space_struct(W.layout)
        row('flow_supg_tau alone, p = %d' % p, timed(
            lambda: _hip.check(lib.flow_supg_tau(
                ctypes.byref(ms), ctypes.byref(ws),
                _hip.f64(conv.data, W.size()), kappa, p, _hip.f64(out),
                _hip.i32(status), _hip.stream()))))
        row('flow_assemble_heat with SUPG alone, P%d' % p,
            timed(heat(V1 if p == 1 else V2, conv, kappa, rho_cp, True)))


if __name__ == '__main__':
    main()
