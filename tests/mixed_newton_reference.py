# -*- coding: utf-8 -*-
'''
The host loop tests/test_mixed_newton_gpu.py compares solve(F == 0, w, bcs) on
a Taylor-Hood space with: dolfin's Newton iteration -- w[dof] = g, then per
step the hand-written Jacobian and the residual at w, the conditions applied
homogeneously, |F|_2, the stopping rule of NEWTON_DEFAULTS, J delta = F, w -=
relaxation * delta -- with scipy's sparse LU on assemble_system(J_hand, None,
bcs).to_scipy() in place of the device's Krylov solve.  The matrices and
residuals are assembled by the package (they are pinned by the tests of mixed
forms); the linear algebra and the loop are the host's.
'''
import numpy
import scipy.sparse.linalg as spla

from flow_amd.fem import assemble, assemble_system, mixed


def bc_dofs(bcs, WP):
    '''(dofs, values) of the conditions in the numbering of WP.'''
    held = mixed.mixed_bcs(bcs, WP)
    if held is None:
        return numpy.zeros(0, dtype=numpy.int64), numpy.zeros(0)
    return held[0].astype(numpy.int64), held[1]


def start(w, bcs):
    '''w[dof] = g, as the solve does first; returns the host copy.'''
    dofs, vals = bc_dofs(bcs, w.function_space())
    x = w.array()
    x[dofs] = vals
    w.set_array(x)
    return x


def residual(F, w, bcs):
    '''F at w with F[dof] = 0 (host array).'''
    dofs, _ = bc_dofs(bcs, w.function_space())
    b = assemble(F).get_local()
    b[dofs] = 0.0
    return b


def newton(F, J_hand, w, bcs, relaxation=1.0, rtol=1.0e-9, atol=1.0e-10,
           maxit=50):
    '''The Newton iteration from the values of w (which it overwrites).
    Returns (iterates, residuals): the host copy of w after w[dof] = g and
    after every step, and |F|_2 before the first and after every step.'''
    x = start(w, bcs)
    iterates, residuals = [x.copy()], []
    while True:
        b = residual(F, w, bcs)
        r = numpy.linalg.norm(b)
        residuals.append(r)
        if r < atol or r / residuals[0] < rtol or len(iterates) > maxit:
            return iterates, residuals
        A, _ = assemble_system(J_hand, None, bcs)
        delta = spla.spsolve(A.to_scipy().tocsc(), b)
        x = x - relaxation * delta
        w.set_array(x)
        iterates.append(x.copy())
