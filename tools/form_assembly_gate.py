# -*- coding: utf-8 -*-
'''
One-off gate for changes to the Python driver of form assembly (fem/ops.py:
newton_jobs, NewtonAssembler, assemble() of ranks 1 and 2): what it plans,
what it computes, how many kernels it launches and what a call costs on the
host, so that two trees can be compared bit for bit.  The same script runs in
both trees; it uses public names only and reads job tuples by position.  The
cases are those of tests/form_assembly_cases.py, which the host test of the
job lists shares.

    python tools/form_assembly_gate.py plan              (host only)
    python tools/form_assembly_gate.py record OUT.npz    (in the old tree)
    python tools/form_assembly_gate.py compare IN.npz    (in the new tree)
    python tools/form_assembly_gate.py time

plan     prints, per case, the jobs of newton_jobs as (kind, signs, (length,
         nout, crc32) of the program, degree, scheme, index of the ds part,
         tag or 0, call or the pair the kind implies).
record   runs every case on UnitSquareMesh(4, 3), P1 and P2: assemble(J) and
         assemble(F) of every Newton case and of the one-shot forms, the held
         NewtonAssembler three times (the state and a Constant changed before
         the second call, the facet markers re-marked before the third), one
         scalar and one vector solve(F == 0); stores every result as an int64
         view and the _hip.launch_count() difference of every call.
compare  does the same and passes when every array is identical as int64 and
         every launch count is equal.
time     wall-clock median of 200 calls (synchronised) of assemble(a),
         assemble(L) and a held NewtonAssembler.assemble() on UnitSquareMesh
         (4, 3), P2, scalar and vector: there the Python driver is the cost.
'''
import os
import sys
import time
import zlib

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

from flow_amd import fem, _hip, device               # noqa: E402
from flow_amd.fem import (                           # noqa: E402
    TestFunction, dx, inner, grad, assemble, ops,
    )

import vector_newton_reference as vnref              # noqa: E402
from form_assembly_cases import (                    # noqa: E402
    all_cases, one_shot_forms, remark, scalar_cases, switches, vector_cases,
    )


# -- plan ------------------------------------------------------------------------
def signature(job, J, F):
    '''A job as plain data; a scalar job of the old planner (6 or 7 entries)
    reads as the nine-field record with part None, tag 0 and no call.'''
    prog = job[3]
    code = repr([tuple(int(x) for x in ins) for ins in prog.code])
    part = job[6] if len(job) > 6 else None
    where = None
    if part is not None:
        parts = [p for _, p in (J if job[0] == 'facet_matrix' else F).terms()]
        where = [i for i, p in enumerate(parts) if p is part][0]
    return (job[0], float(job[1]), float(job[2]),
            (len(prog.code), prog.nout, zlib.crc32(code.encode()) & 0xffffffff),
            job[4], job[5], where, job[7] if len(job) > 7 else 0,
            tuple(job[8]) if len(job) > 8 else None)


def plan():
    switches()
    mesh = fem.UnitSquareMesh(4, 3)
    for case in all_cases(mesh):
        jobs = ops.newton_jobs(case.J, case.F, fuse=case.fuse)
        print('%s:' % case.name)
        for job in jobs:
            print('    %r,' % (signature(job, case.J, case.F),))


# -- record / compare --------------------------------------------------------------
class Log(object):
    def __init__(self):
        self.data = {}

    def array(self, key, t):
        a = t.detach().cpu().numpy() if hasattr(t, 'detach') else \
            numpy.asarray(t, dtype=numpy.float64)
        assert key not in self.data, key
        self.data[key] = numpy.ascontiguousarray(a).view(numpy.int64).copy()

    def count(self, key, n):
        assert key not in self.data, key
        self.data[key] = numpy.array([n], dtype=numpy.int64)

    def call(self, key, fn):
        n0 = _hip.launch_count()
        out = fn()
        self.count(key + ' launches', _hip.launch_count() - n0)
        return out


def result(x):
    return x.vals if hasattr(x, 'vals') else x.data if hasattr(x, 'data') \
        and not hasattr(x, 'numel') else x


def run_all():
    switches()
    log = Log()
    mesh = fem.UnitSquareMesh(4, 3)
    for name, form, fcp in one_shot_forms(mesh):
        for turn in range(2):
            key = 'assemble %s #%d' % (name, turn)
            log.array(key, result(log.call(key, lambda: assemble(
                form, form_compiler_parameters=fcp))))
    for case in all_cases(mesh):
        for what, form in (('J', case.J), ('F', case.F)):
            key = 'assemble %s of %s' % (what, case.name)
            log.array(key, result(log.call(key, lambda: assemble(form))))
        asm = ops.NewtonAssembler(case.J, case.F, case.V, fuse=case.fuse)
        log.count('fused ' + case.name, int(asm.fused))
        u0 = case.u.array().copy()
        c0 = case.const.values().copy()
        for turn in range(3):
            if turn == 1:
                case.u.set_array(u0 * 1.25 + 0.125)
                case.const.assign(c0 * 1.5)
            if turn == 2 and case.markers is not None:
                remark(case.markers)
            key = 'held %s #%d' % (case.name, turn)
            A, b = log.call(key, asm.assemble)
            log.array(key + ' A', A.vals)
            log.array(key + ' b', b)
        case.u.set_array(u0)
        case.const.assign(c0)
    # one scalar and one vector solve(F == 0)
    V = fem.FunctionSpace(mesh, 'CG', 2)
    u, v = fem.Function(V), TestFunction(V)
    f = fem.Expression('10.0*sin(3.0*x[0]) + x[1]', degree=2)
    F = (1 + u**2) * inner(grad(u), grad(v)) * dx - f * v * dx
    solves = [('scalar', u, F, [fem.DirichletBC(V, 0.0, 'on_boundary')])]
    W, uw, Fw, bcs, _ = vnref.burgers_problem(4, 2)
    solves.append(('vector', uw, Fw, bcs))
    for name, u, F, bcs in solves:
        key = 'solve ' + name
        info = log.call(key, lambda: fem.solve(F == 0, u, bcs))
        log.array(key + ' residuals', info.residuals)
        log.count(key + ' linear iterations',
                  sum((i + 1) * n for i, n in enumerate(info.linear_iterations)))
        log.count(key + ' method', zlib.crc32(info.method.encode()))
        log.count(key + ' fused', int(info.fused))
        log.array(key + ' u', u.data)
    device.synchronize()
    return log.data


def compare(path):
    want = numpy.load(path)
    got = run_all()
    bad = sorted(set(want.files) ^ set(got))
    arrays = calls = 0
    for key in sorted(set(want.files) & set(got)):
        same = want[key].shape == got[key].shape and \
            numpy.array_equal(want[key], got[key])
        if key.endswith(' launches'):
            calls += 1
        elif want[key].size > 1 or ' A' in key or ' b' in key:
            arrays += 1
        if not same:
            bad.append(key)
            print('DIFFERS: %s  %s -> %s' % (
                key, want[key] if want[key].size < 4 else want[key].shape,
                got[key] if got[key].size < 4 else got[key].shape))
    print('compared %d entries: %d arrays, %d launch counts, %d other figures'
          % (len(got), arrays, calls, len(got) - arrays - calls))
    if bad:
        print('FAILED: %d entries differ or are missing' % len(bad))
        return 1
    print('PASSED: every array identical as int64, every launch count equal')
    return 0


# -- time ------------------------------------------------------------------------
def median_us(call, repeat=200, warmup=20):
    for _ in range(warmup):
        call()
    device.synchronize()
    out = []
    for _ in range(repeat):
        t = time.perf_counter()
        call()
        device.synchronize()
        out.append(time.perf_counter() - t)
    return 1e6 * float(numpy.median(out))


def host_times():
    switches()
    mesh = fem.UnitSquareMesh(4, 3)
    V = fem.FunctionSpace(mesh, 'CG', 2)
    W = fem.VectorFunctionSpace(mesh, 'CG', 2)
    for name, case in (('scalar', list(scalar_cases(mesh, V))[0]),
                       ('vector', list(vector_cases(mesh, W))[0])):
        asm = ops.NewtonAssembler(case.J, case.F, case.V)
        for what, call in (('assemble(a)', lambda: assemble(case.J)),
                           ('assemble(L)', lambda: assemble(case.F)),
                           ('held assemble()', asm.assemble)):
            print('time %s %-16s %9.1f us' % (name, what, median_us(call)))


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else ''
    if mode == 'plan':
        plan()
    elif mode == 'record':
        numpy.savez(sys.argv[2], **run_all())
        print('recorded %s' % sys.argv[2])
    elif mode == 'compare':
        sys.exit(compare(sys.argv[2]))
    elif mode == 'time':
        host_times()
    else:
        sys.exit(__doc__)


if __name__ == '__main__':
    main()
