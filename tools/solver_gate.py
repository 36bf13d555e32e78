# -*- coding: utf-8 -*-
'''
One-off gate for changes to the host side of the Krylov drivers (flow_amd/csrc/
krylov_kernels.hip): what the solvers return, bit for bit, how many kernels
they launch and what a launch-bound solve costs on the host, so that two
builds of the library can be compared.  The same script runs in both trees
(copy it into the old one); it uses public names only.

    python tools/solver_gate.py record OUT.npz    (in the old tree)
    python tools/solver_gate.py compare IN.npz    (in the new tree)
    python tools/solver_gate.py time OTHER.so     (in the new tree)

record   UnitSquareMesh(12, 10), P1 and P2: CG plain, with Jacobi, the two-level
         and the multigrid preconditioner; guarded CG from a good start, a bad
         one, and a bad one with a bad fallback; BiCGStab and GMRES on a
         perturbed 2x2-block system without a preconditioner, with Jacobi and
         with ILU(0); GMRES with x_is_zero set and unset, restart 3 (so that
         it restarts), verify on and off; the matrix-free operator through one
         rotational step of the small channel case (Newton-GMRES).  Stores x
         as an int64 view, iterations, residual, starts_dropped and the
         _hip.launch_count() difference of every solve.
compare  does the same and passes when every entry is equal.
time     host time per solve of the 25-row cases of tests/
         test_solver_verdicts_gpu.py, this tree's library and OTHER.so
         alternated in one process: median and min-max of 200 solves each.
'''
import ctypes
import os
import sys
import time

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

from flow_amd import fem, _hip, device               # noqa: E402
from flow_amd.fem import ops, ilu                    # noqa: E402
from flow_amd.fem.multigrid import Multigrid         # noqa: E402


def dev(a):
    return device.to_device(numpy.ascontiguousarray(a, dtype=numpy.float64))


class Log(object):
    def __init__(self):
        self.data = {}

    def put(self, key, a):
        assert key not in self.data, key
        a = a.detach().cpu().numpy() if hasattr(a, 'detach') else \
            numpy.atleast_1d(numpy.asarray(a, dtype=numpy.float64))
        self.data[key] = numpy.ascontiguousarray(a).view(numpy.int64).copy()

    def solve(self, key, method, A, b, x0, **kw):
        x = dev(numpy.zeros(A.size) if x0 is None else x0)
        n0 = _hip.launch_count()
        info = ops.krylov_solve(method, A, dev(b), x, **kw)
        self.put(key + ' launches', _hip.launch_count() - n0)
        self.put(key + ' x', x)
        self.put(key + ' figures', [info.iterations, info.residual,
                                    getattr(info, 'starts_dropped', 0)])
        return x.cpu().numpy()


def block_system(V, rng):
    '''The perturbed 2x2-block system of tests/test_hip_parity.py.'''
    import torch
    M = ops.assemble_mass(V).vals
    K = ops.assemble_stiffness(V).vals
    pert = dev(0.02 * rng.standard_normal(4 * M.numel()) * float(M.abs().max()))
    base = torch.cat([M + 0.01 * K, torch.zeros_like(M), torch.zeros_like(M),
                      M + 0.01 * K])
    return ops.Matrix(V.layout, 2, (base + pert).contiguous())


def run_all():
    log = Log()
    mesh = fem.UnitSquareMesh(12, 10)
    for deg in (1, 2):
        tag = 'P%d ' % deg
        rng = numpy.random.RandomState(40 + deg)
        V = fem.FunctionSpace(mesh, 'CG', deg)
        n = V.N
        M = ops.assemble_mass(V)
        b = rng.standard_normal(n)
        log.solve(tag + 'cg plain', 'cg', M, b, None, rtol=1e-10, dinv=None,
                  check_every=7)
        xs = log.solve(tag + 'cg jacobi', 'cg', M, b, None, rtol=1e-11,
                       first_check=3, check_every=2)
        if deg == 1:
            isbc = mesh.points[:, 0] > 1.0 - 1e-12
            K = ops.symmetric_bc_matrix(
                ops.assemble_stiffness(V),
                device.to_device(isbc.astype(numpy.uint8)))
            bk = b.copy()
            bk[isbc] = 0.0
            coarse = ops.CoarseSpace(K, isbc, singular=False, target_nc=16)
            log.solve(tag + 'cg two-level', 'cg', K, bk, None, rtol=1e-10,
                      coarse=coarse, check_every=5)
            mg = Multigrid(K, isbc, coarsest=20)
            log.put(tag + 'mg levels', mg.nlevels)
            assert mg.nlevels >= 2
            log.solve(tag + 'cg multigrid', 'cg', K, bk, None, rtol=1e-10,
                      mg=mg, check_every=4)
        noise = rng.standard_normal(n)
        good, far = xs + 1e-3 * noise, 1.0e6 * noise
        for name, x0, guard in (('good start', good, False),
                                ('bad start', far, False),
                                ('bad start, good fallback', far, dev(good)),
                                ('bad start, bad fallback', far, dev(-far))):
            log.solve(tag + 'guarded cg ' + name, 'cg', M, b, x0, rtol=1e-10,
                      guard=guard, check_every=3)
        A = block_system(V, rng)
        b2 = rng.standard_normal(2 * n)
        x2 = rng.standard_normal(2 * n)
        pres = (('none', dict(dinv=None)), ('jacobi', dict()),
                ('ilu', dict(ilu=ilu.Ilu0(A, packed=True, single_vector=True))))
        for pname, kw in pres:
            log.solve(tag + 'bicgstab ' + pname, 'bicgstab', A, b2, None,
                      rtol=1e-10, check_every=3, first_check=2, **kw)
            for zero in (True, False):
                for restart in (20, 3):
                    for verify in (True, False):
                        key = tag + 'gmres %s zero=%d restart=%d verify=%d' % (
                            pname, zero, restart, verify)
                        log.solve(key, 'gmres', A, b2, None if zero else x2,
                                  rtol=1e-10, maxit=400, restart=restart,
                                  x_is_zero=zero, verify=verify,
                                  first_check=4 if verify else 0, **kw)
    # the matrix-free Jacobian action: one step of the small channel case
    import cases
    case = cases.Case(fem.karman_channel(30, 10, fitted=True), vdeg=2, dt=0.02,
                      bc_kind='channel', rho=1.5, mu=0.05, seed=1)
    n0 = _hip.launch_count()
    u1, p1, ui = case.product_step('rotational')
    log.put('channel step launches', _hip.launch_count() - n0)
    for name, a in (('u1', u1), ('p1', p1), ('ui', ui)):
        log.put('channel step ' + name, numpy.asarray(a, dtype=numpy.float64))
    device.synchronize()
    return log.data


def compare(path):
    want = numpy.load(path)
    got = run_all()
    bad = sorted(set(want.files) ^ set(got))
    for key in sorted(set(want.files) & set(got)):
        if want[key].shape != got[key].shape or \
                not numpy.array_equal(want[key], got[key]):
            bad.append(key)
            print('DIFFERS: %s' % key)
    solves = sum(1 for k in got if k.endswith(' launches'))
    print('compared %d entries of %d solves' % (len(got), solves))
    if bad:
        print('FAILED: %d entries differ or are missing: %s' % (len(bad), bad))
        return 1
    print('PASSED: every x identical as int64; iterations, residuals, '
          'starts_dropped and launch counts equal')
    return 0


# -- time ------------------------------------------------------------------------
def other_library(path):
    lib = ctypes.CDLL(path)
    lib.flow_last_error.restype = ctypes.c_char_p
    lib.flow_last_error.argtypes = []
    for name, argtypes in _hip.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = argtypes
    assert lib.flow_abi_version() == _hip.ABI_VERSION
    return lib


def host_times(other_path, repeat=200, warmup=20):
    mesh = fem.UnitSquareMesh(4, 4)
    M = ops.assemble_mass(fem.FunctionSpace(mesh, 'CG', 1))
    n = M.size
    dinv = M.diag_inv()
    rng = numpy.random.RandomState(11)
    b = dev(rng.standard_normal(n))
    x = device.zeros(n)
    libs = (('this', _hip.lib()), ('other', other_library(other_path)))
    rows = []
    for method in ('cg', 'bicgstab', 'gmres'):
        for name, kw in (('one batch', dict(check_every=50, first_check=50)),
                         ('every iteration', dict(check_every=1,
                                                  first_check=1))):
            def call():
                x.zero_()
                ops.krylov_solve(method, M, b, x, 1e-10, maxit=100, dinv=dinv,
                                 **kw)
            t = {'this': [], 'other': []}
            for i in range(warmup + repeat):
                for which, lib in libs:
                    _hip._LIB = lib
                    device.synchronize()
                    t0 = time.perf_counter()
                    call()
                    device.synchronize()
                    if i >= warmup:
                        t[which].append(1e6 * (time.perf_counter() - t0))
            _hip._LIB = libs[0][1]
            row = ['%s, %s' % (method, name)]
            for which in ('other', 'this'):
                a = numpy.array(t[which])
                row += [float(numpy.median(a)), float(a.min()), float(a.max())]
            rows.append(row)
            print('time %-26s other: median %8.1f us (min %8.1f, max %8.1f)  '
                  'this: median %8.1f us (min %8.1f, max %8.1f)' % tuple(row))
    return rows


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else ''
    if mode == 'record':
        numpy.savez(sys.argv[2], **run_all())
        print('recorded %s' % sys.argv[2])
    elif mode == 'compare':
        sys.exit(compare(sys.argv[2]))
    elif mode == 'time':
        host_times(sys.argv[2])
    else:
        sys.exit(__doc__)


if __name__ == '__main__':
    main()
