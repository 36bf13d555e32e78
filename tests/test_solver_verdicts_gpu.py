# -*- coding: utf-8 -*-
'''
How the Krylov drivers end (flow_amd/csrc/krylov_kernels.hip: run_batches for
CG and BiCGStab, gmres_cycle for GMRES): the verdict the host reads behind a
batch of enqueued iterations -- converged, start rejected, out of iterations,
not a number -- with the iteration count, the return code and the message
each one carries.  One 25-row system: the P1 mass matrix of UnitSquareMesh(4,
4), Jacobi-preconditioned.  GPU only; a second in all.
'''
import numpy
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1.0e-10
METHODS = ('cg', 'bicgstab', 'gmres')
# (solver name, residual label) as the messages spell them
NAMES = {'cg': ('CG', r'\|B r\|'), 'bicgstab': ('BiCGStab', r'\|r\|'),
         'gmres': ('GMRES', r'\|r\|')}


class System(object):
    def __init__(self):
        from flow_amd import fem, device
        from flow_amd.fem import ops
        mesh = fem.UnitSquareMesh(4, 4)
        self.M = ops.assemble_mass(fem.FunctionSpace(mesh, 'CG', 1))
        self.n = self.M.size
        assert self.n == 25
        self.dinv = self.M.diag_inv()
        rng = numpy.random.RandomState(11)
        self.b_host = rng.standard_normal(self.n)
        self.b = device.to_device(self.b_host)
        self.noise = rng.standard_normal(self.n)
        # the solution, for the starts of the guarded solves
        x = device.zeros(self.n)
        ops.krylov_solve('cg', self.M, self.b, x, 1e-13, dinv=self.dinv)
        self.x_host = x.cpu().numpy().copy()

    def solve(self, method, b=None, x0=None, **kw):
        '''(info, x on the host) of one solve from x0 (default: zero).'''
        from flow_amd import device
        from flow_amd.fem import ops
        x = device.zeros(self.n) if x0 is None else device.to_device(x0)
        kw.setdefault('maxit', 100)
        info = ops.krylov_solve(method, self.M, self.b if b is None else b, x,
                                kw.pop('rtol', RTOL), dinv=self.dinv, **kw)
        return info, x.cpu().numpy().copy()

    def defect(self, x_host):
        from flow_amd import device
        y = device.zeros(self.n)
        self.M.apply(device.to_device(x_host), y)
        return float(numpy.linalg.norm(y.cpu().numpy() - self.b_host) /
                     numpy.linalg.norm(self.b_host))


@pytest.fixture(scope='module')
def system(hip):
    return System()


@pytest.mark.parametrize('method', METHODS)
def test_converges_in_the_first_batch_and_in_a_later_one(system, method):
    '''One large batch and read-backs after every iteration stop at the same
    iterate: the same count, the same solution bit for bit (the device
    freezes it; the host only finds out later).'''
    big, x_big = system.solve(method, check_every=50, first_check=50)
    assert 1 < big.iterations < 50
    assert big.residual > 0.0
    # (the stopping tests are relative to |b| or |B b|; kappa(D^-1 M) < 10)
    assert system.defect(x_big) < 100 * RTOL
    small, x_small = system.solve(method, check_every=1, first_check=1)
    assert small.iterations == big.iterations
    assert small.residual == big.residual
    assert numpy.array_equal(x_small.view(numpy.int64), x_big.view(numpy.int64))


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('maxit', (1, 0))
def test_out_of_iterations(system, method, maxit):
    from flow_amd import _hip
    name, label = NAMES[method]
    with pytest.raises(_hip.NotConverged,
                       match=r'^%s did not converge in %d iterations: %s = '
                             r'\d\.\d{3}e[-+]\d\d > \d\.\d{3}e[-+]\d\d$'
                             % (name, maxit, label)):
        system.solve(method, maxit=maxit, check_every=1)


@pytest.mark.parametrize('method', METHODS)
def test_no_iterations_needed(system, method):
    '''maxit = 0 with a start that passes the test already: converged, zero
    iterations, x untouched.'''
    info, x = system.solve(method, x0=system.x_host, rtol=1e-6, maxit=0)
    assert info.iterations == 0
    assert numpy.array_equal(x, system.x_host)


@pytest.mark.parametrize('method', METHODS)
def test_not_a_number_breaks_down(system, method):
    '''A NaN in the right-hand side is a numerical input: the solve ends with
    FLOW_NOT_CONVERGED and says so.'''
    from flow_amd import _hip, device
    bad = system.b_host.copy()
    bad[3] = numpy.nan
    with pytest.raises(_hip.NotConverged,
                       match=r'^%s broke down \(NaN( residual)?\) at '
                             r'iteration \d+$' % NAMES[method][0]):
        system.solve(method, b=device.to_device(bad), check_every=1)
    # ... and the next solve on the same stream is sound
    info, x = system.solve(method)
    assert system.defect(x) < 100 * RTOL


def test_guarded_cg_counts_the_starts_it_drops(system):
    from flow_amd import device
    good = system.x_host + 1e-3 * system.noise
    far = 1.0e6 * system.noise
    ref, _ = system.solve('cg', x0=good)
    assert getattr(ref, 'starts_dropped', 0) == 0
    for x0, guard, dropped in ((good, False, 0),
                               (far, False, 1),
                               (far, device.to_device(good), 1),
                               (far, device.to_device(-far), 2)):
        info, x = system.solve('cg', x0=x0, guard=guard)
        assert info.starts_dropped == dropped
        assert system.defect(x) < 100 * RTOL
    # a kept start: the unguarded solve's count; the good fallback as well
    info, _ = system.solve('cg', x0=good, guard=False)
    assert info.iterations == ref.iterations
    info, _ = system.solve('cg', x0=far, guard=device.to_device(good))
    assert info.iterations == ref.iterations
