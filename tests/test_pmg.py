# -*- coding: utf-8 -*-
'''
The p-multigrid / Chebyshev preconditioner of the Newton systems
(flow_amd/fem/pmg.py, flow_amd/csrc/pmg_kernels.hip): transfer tables on the
CPU; on the GPU one application against a numpy restatement of the cycle built
from the same matrices, the spectral-radius estimate, and GMRES with it against
a direct solve and against the multicolour ILU(0).
'''
import numpy
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from flow_amd import fem
from flow_amd.fem.pmg import transfer_tables
from flow_amd.fem.space import scalar_layout

import cases


def _prolongation(lay2):
    ends, rptr, rsrc = transfer_tables(lay2)
    n, n1 = lay2.N, lay2.mesh.num_vertices()
    rows = numpy.repeat(numpy.arange(n), 2)
    P = sp.csr_matrix((numpy.full(2 * n, 0.5), (rows, ends.ravel())),
                      shape=(n, n1))
    return P, ends, rptr, rsrc


@pytest.mark.parametrize('fitted', [False, True])
def test_transfer_tables_embed_p1_in_p2(fitted):
    mesh = fem.karman_channel(36, 12, fitted=fitted)
    lay2 = scalar_layout(mesh, 2)
    lay1 = scalar_layout(mesh, 1)
    P, ends, rptr, rsrc = _prolongation(lay2)
    # a P1 function is reproduced at every P2 node
    f = lambda x: 0.3 - 1.7 * x[:, 0] + 2.9 * x[:, 1]
    assert abs(P.dot(f(lay1.dof_coords)) - f(lay2.dof_coords)).max() < 1e-13
    # the restriction lists are the transpose: own dof first (weight 1), then
    # the edge dofs (weight 1/2)
    R = P.T.tocsr()
    n1 = lay1.N
    assert rptr[0] == 0 and rptr[-1] == len(rsrc) and len(rptr) == n1 + 1
    for v in (0, 1, n1 // 2, n1 - 1):
        own, others = rsrc[rptr[v]], rsrc[rptr[v] + 1:rptr[v + 1]]
        assert own == lay2.vertex_dofs[v]
        row = R.getrow(v)
        want = dict(zip(row.indices, row.data))
        assert want.pop(own) == 1.0
        assert sorted(want) == sorted(others)
        assert all(w == 0.5 for w in want.values())
    x = numpy.random.RandomState(0).standard_normal(lay2.N)
    got = numpy.array([x[rsrc[rptr[v]]]
                       + 0.5 * x[rsrc[rptr[v] + 1:rptr[v + 1]]].sum()
                       for v in range(n1)])
    assert abs(got - R.dot(x)).max() < 1e-13


@pytest.mark.parametrize('world', [2, 3, 8])
def test_block_transfer_tables_are_the_diagonal_blocks(world):
    '''The strips use the cycle rank-locally (block Jacobi): the tables of a
    rank are the diagonal block P[r0:r1, v0:v1] of the global prolongation in
    local numbering -- an end point outside the block names the dummy coarse
    row, the restriction lists are the transpose of exactly that block -- and
    the level's local CSR keeps the pattern of its rows with the couplings
    that leave the block marked (keep = 0, column = own row).'''
    from flow_amd import parallel
    from flow_amd.fem.pmg import local_transfer_tables
    mesh = fem.karman_channel(120, 30, fitted=True)
    lay2 = scalar_layout(mesh, 2)
    lay1 = scalar_layout(mesh, 1)
    P = _prolongation(lay2)[0]
    st = parallel.Strips(mesh, world)
    b2, b1 = st.blocks(lay2), st.blocks(lay1)
    rp = lay2.pattern('rowptr').astype(numpy.int64)
    cols = lay2.pattern('cols').astype(numpy.int64)
    for g in range(world):
        (r0, r1), (v0, v1) = b2.rows(g), b1.rows(g)
        n, n1 = r1 - r0, v1 - v0
        ends, rptr, rsrc = local_transfer_tables(lay2, (r0, r1), (v0, v1))
        assert ends.shape == (n, 2) and ends.min() >= 0 and ends.max() <= n1
        rows = numpy.repeat(numpy.arange(n), 2)
        Ploc = sp.csr_matrix((numpy.full(2 * n, 0.5), (rows, ends.ravel())),
                             shape=(n, n1 + 1))[:, :n1]          # drop the dummy
        want = P[r0:r1, v0:v1]
        assert abs(Ploc - want).max() == 0.0
        # restriction lists = transpose of the block, own dof first
        R = sp.lil_matrix((n1, n))
        for v in range(n1):
            lst = rsrc[rptr[v]:rptr[v + 1]]
            assert lst[0] == lay2.vertex_dofs[v0 + v] - r0
            R[v, lst[0]] = 1.0
            for i in lst[1:]:
                R[v, i] = 0.5
        assert abs(R.tocsr() - want.T).max() == 0.0
    # the level's local pattern (host tables only: no device needed)
    g = world - 1
    r0, r1 = b2.rows(g)
    seg = cols[rp[r0]:rp[r1]]
    inside = (seg >= r0) & (seg < r1)
    assert inside.sum() < len(seg)              # couplings across the strip edge
    row_of = numpy.repeat(numpy.arange(r0, r1), numpy.diff(rp[r0:r1 + 1]))
    assert (row_of[~inside] < r1).all()


# -- numpy restatement of one application -------------------------------------------
def _cheb(A, D, lo, hi, k, r, x=None):
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    sigma = theta / delta
    rho = 1.0 / sigma
    if x is None:
        x = numpy.zeros_like(r)
        res = r.copy()
    else:
        res = r - A.dot(x)
    d = res / D / theta
    for j in range(k):
        x = x + d
        if j + 1 < k:
            res = res - A.dot(d)
            rn = 1.0 / (2.0 * sigma - rho)
            d = rn * rho * d + 2.0 * rn / delta * res / D
            rho = rn
    return x


def _one_plane(Ms, n):
    """flow_pmg_pack1 (pmg_kernels.hip) in numpy: the operators the one-plane
    levels apply to component 0 and 1 -- ONE plane, the mean of the diagonal
    blocks over the components in which neither the row nor the column is a
    Dirichlet dof, plus the identity rows of each component."""
    B = [Ms[a * n:(a + 1) * n, a * n:(a + 1) * n].tocsr() for a in (0, 1)]
    free = []
    for Ba in B:
        off = Ba - sp.diags(Ba.diagonal())
        off.eliminate_zeros()
        free.append((numpy.diff(off.tocsr().indptr) > 0).astype(float))
    S = (abs(B[0]) + abs(B[1])).tocsr()
    S.data[:] = 1.0
    U = [sp.diags(f).dot(Ba).dot(sp.diags(f)) for f, Ba in zip(free, B)]
    cnt = sum(sp.diags(f).dot(S).dot(sp.diags(f)) for f in free).tocsr()
    cnt.eliminate_zeros()
    inv = cnt.copy()
    inv.data = 1.0 / inv.data
    plane = (U[0] + U[1]).multiply(inv).tocsr()
    return [(sp.diags(f).dot(plane)
             + sp.diags((1.0 - f) * Ba.diagonal())).tocsr()
            for f, Ba in zip(free, B)]


def _cycle(pre, A, A1, P, bc0, bc1, r):
    '''One component of flow_pmg_apply in fp64.'''
    f, c = pre.fine.struct, pre.coarse.struct
    s = pre.struct
    D, D1 = A.diagonal(), A1.diagonal()
    x = _cheb(A, D, f.lam_min, f.lam_max, s.pre, r)
    rc = P.T.dot(r - A.dot(x))
    rc[bc1] = 0.0
    x = x + P.dot(_cheb(A1, D1, c.lam_min, c.lam_max, s.coarse_steps, rc))
    x = _cheb(A, D, f.lam_min, f.lam_max, s.post, r, x)
    x[bc0] = r[bc0]
    return x


def _fgmres_count(J, b, prec, rtol=1e-8, restart=10, maxit=300):
    '''Applications a right-preconditioned flexible GMRES(restart) needs.'''
    n = len(b)
    x = numpy.zeros(n)
    bn = numpy.linalg.norm(b)
    its = 0
    while its < maxit:
        r = b - J.dot(x)
        beta = numpy.linalg.norm(r)
        if beta <= rtol * bn:
            break
        V = [r / beta]
        Z = []
        Hm = numpy.zeros((restart + 1, restart))
        g = numpy.zeros(restart + 1)
        g[0] = beta
        for j in range(restart):
            Z.append(prec(V[j]))
            w = J.dot(Z[j])
            for i in range(j + 1):
                Hm[i, j] = w.dot(V[i])
                w = w - Hm[i, j] * V[i]
            Hm[j + 1, j] = numpy.linalg.norm(w)
            V.append(w / Hm[j + 1, j])
            its += 1
            y = numpy.linalg.lstsq(Hm[:j + 2, :j + 1], g[:j + 2], rcond=None)[0]
            res = numpy.linalg.norm(g[:j + 2] - Hm[:j + 2, :j + 1].dot(y))
            if res <= rtol * bn or its >= maxit:
                break
        x = x + numpy.array(Z[:len(y)]).T.dot(y)
        if res <= rtol * bn:
            break
    return its


def test_the_cycle_as_an_algorithm_on_the_oracles_jacobian():
    '''The preconditioner as mathematics, without a GPU: the oracle's Jacobian
    of a body-fitted channel in the non-dimensional regime of the 10 M-DoF
    workload (viscosity scaled with the mesh width: cell Peclet ~2, CFL ~1.8,
    diffusion number ~0.85), the P1 discretisation of the same operator as
    coarse level through the product's transfer tables, the default cycle
    (1 + 2 Chebyshev steps on P2 and 6 on P1; the numpy restatement above, in
    fp64): one application
    contracts a random vector, and flexible GMRES needs about a third of the
    applications Jacobi needs (tools/precond_lab.py: 132 / 34 / 14 for Jacobi /
    multicolour ILU(0) / this cycle at 300 x 70).'''
    from types import SimpleNamespace
    import flow_amd.navier_stokes as navsto
    from flow_amd import karman
    from flow_amd.fem.bcs import collect
    from flow_amd.fem import reference
    from oracle import fem_oracle as orc
    import oracle_harness as H
    nx = 72
    prob = karman.KarmanProblem(nx)
    mesh = prob.mesh
    lay2, lay1 = prob.W.layout, prob.P.layout
    n, n1 = lay2.N, lay1.N
    W2, W1, Po = (H.oracle_space(mesh, 2), H.oracle_space(mesh, 1),
                  H.oracle_space(mesh, 1))
    rho, mu = prob.rho, 0.002 * 2182.0 / nx
    dt = mesh.hmax() / 0.0159
    bc, vals = collect(prob.u_bcs, 2 * n)
    # a divergence-free-ish state: the inflow profile, zero on the obstacle
    prob.set_initial_profile()
    u = prob.u0.array().copy()
    u[bc] = vals
    zero = (reference.lattice(0), numpy.zeros((mesh.num_cells(), 1, 2)))
    p0 = numpy.zeros(n1)

    def jacobian(Wo, uu, bcd):
        _, dR = orc.momentum_rhs(Wo, Po, uu, p0, zero, rho, mu)
        M = sp.block_diag([orc.mass_matrix(Wo)] * 2, format='csr')
        Jm = (M - dt / rho * dR).tocsr()
        keep = numpy.ones(Jm.shape[0])
        keep[bcd] = 0.0
        return (sp.diags(keep).dot(Jm) + sp.diags(1.0 - keep)).tocsr()
    J = jacobian(W2, u, bc)
    vd = lay2.vertex_dofs
    vertex_of = numpy.full(n, -1)
    vertex_of[vd] = numpy.arange(n1)
    comp, row = bc // n, bc % n
    sel = vertex_of[row] >= 0
    bc1 = comp[sel] * n1 + vertex_of[row[sel]]
    J1 = jacobian(W1, numpy.concatenate([u[:n][vd], u[n:][vd]]), bc1)
    P = _prolongation(lay2)[0]
    isbc0 = numpy.zeros(2 * n, dtype=bool)
    isbc0[bc] = True
    isbc1 = numpy.zeros(2 * n1, dtype=bool)
    isbc1[bc1] = True

    def lam_max(A):
        v = numpy.random.RandomState(3).standard_normal(A.shape[0])
        d = A.diagonal()
        for _ in range(25):
            v = A.dot(v) / d
            lam = numpy.linalg.norm(v)
            v /= lam
        return lam

    def block(a):
        A = J[a * n:(a + 1) * n, a * n:(a + 1) * n].tocsr()
        A1 = J1[a * n1:(a + 1) * n1, a * n1:(a + 1) * n1].tocsr()
        l0, l1 = lam_max(A), lam_max(A1)
        # (the cycle the solver runs by default)
        par = navsto.solver_parameters['newton']['pmg']
        pre = SimpleNamespace(
            fine=SimpleNamespace(struct=SimpleNamespace(
                lam_min=l0 / par['ratio_fine'], lam_max=1.1 * l0)),
            coarse=SimpleNamespace(struct=SimpleNamespace(
                lam_min=l1 / par['ratio_coarse'], lam_max=1.1 * l1)),
            struct=SimpleNamespace(pre=par['pre'], post=par['post'],
                                   coarse_steps=par['coarse_steps']))
        return lambda r: _cycle(pre, A, A1, P, isbc0[a * n:(a + 1) * n],
                                isbc1[a * n1:(a + 1) * n1], r)
    cyc = [block(0), block(1)]
    cycle = lambda r: numpy.concatenate([cyc[0](r[:n]), cyc[1](r[n:])])
    v = numpy.random.RandomState(7).standard_normal(2 * n)
    v[bc] = 0.0
    contraction = numpy.linalg.norm(v - cycle(J.dot(v))) / numpy.linalg.norm(v)
    assert contraction < 0.5, contraction
    b = numpy.random.RandomState(1).standard_normal(2 * n)
    b[bc] = 0.0
    d = J.diagonal()
    its_jacobi = _fgmres_count(J, b, lambda r: r / d)
    its_cycle = _fgmres_count(J, b, cycle)
    print('contraction %.2f, FGMRES(10) to 1e-8: Jacobi %d, cycle %d'
          % (contraction, its_jacobi, its_cycle))
    assert its_cycle <= 20 and 3 * its_cycle < its_jacobi, (its_cycle, its_jacobi)


@pytest.fixture(scope='module')
def newton_system(hip):
    '''A Karman problem after two CFL-sized steps with the p-multigrid: the
    assembled Jacobians of both levels and the preconditioner built from
    them.'''
    from flow_amd import karman
    import flow_amd.navier_stokes as navsto
    old = navsto.solver_parameters['newton']['preconditioner']
    navsto.solver_parameters['newton']['preconditioner'] = 'pmg'
    try:
        prob = karman.KarmanProblem(160, 37, mu=0.02)
        prob.set_initial_profile()
        prob.dt = prob.hmax / 0.016
        infos = [prob.step(adapt=False) for _ in range(2)]
    finally:
        navsto.solver_parameters['newton']['preconditioner'] = old
    lay = prob.W.layout
    pre = lay._dev['jacobian_pmg']
    # the cycle contracts here (cell Peclet number ~2, as on the 10 M-DoF
    # workload) and was accepted
    assert pre.contraction < 0.6 and 'pmg_rejected' not in lay._dev
    J = lay._dev['jacobian']
    J1 = lay._dev['pmg_coarse']['J1']
    return prob, infos, pre, J, J1


@pytest.mark.gpu
def test_falls_back_to_ilu_where_the_cycle_does_not_contract(hip):
    '''The same channel with the physical viscosity on a coarse mesh: cell
    Peclet number ~30 with a Galerkin discretisation.  Chebyshev smoothing
    assumes a spectrum near the real axis; here the cycle amplifies, the
    contraction test sees it, and the step runs with the ILU(0).'''
    from flow_amd import karman
    import flow_amd.navier_stokes as navsto
    assert navsto.solver_parameters['newton']['preconditioner'] == 'pmg'
    prob = karman.KarmanProblem(150, 35)
    prob.set_initial_profile()
    prob.dt = prob.hmax / 0.016
    infos = [prob.step(adapt=False) for _ in range(2)]
    lay = prob.W.layout
    # (what replaces it: the two-level ILU cycle, or -- by its own self-test
    # -- the bare ILU(0) whose factors it holds)
    assert 'pmg_rejected' in lay._dev and 'jacobian_tl' in lay._dev
    assert infos[0]['newton_preconditioner'] in ('tlilu', 'ilu0')
    assert not infos[0]['pmg_contraction'] < 0.8
    for i in infos:
        assert i['newton_residuals'][-1] < 1e-10
    # a tiny step is mass-dominated: the rejection lapses and the cycle is
    # accepted again
    prob.dt = 1.0e-3 * prob.dt
    info = prob.step(adapt=False)
    assert info['pmg_contraction'] < 0.8


@pytest.mark.gpu
def test_one_application_matches_the_numpy_cycle(newton_system):
    from flow_amd import device
    prob, infos, pre, J, J1 = newton_system
    lay = prob.W.layout
    n, n1 = lay.N, pre.lay1.N
    Js, J1s = J.to_scipy().tocsr(), J1.to_scipy().tocsr()
    P = _prolongation(lay)[0]
    bc0 = device.to_host(pre._keep['bc_fine']).numpy().astype(bool)
    bc1 = device.to_host(pre._keep['bc_coarse']).numpy().astype(bool)
    assert bc0.sum() > 0 and bc1.sum() > 0
    # the Dirichlet rows are identity rows on both levels
    for M, m in ((Js, bc0), (J1s, bc1)):
        rows = numpy.nonzero(m)[0]
        sub = M[rows]
        assert abs(sub.dot(numpy.ones(M.shape[1])) - 1.0).max() == 0.0
    A = [Js[a * n:(a + 1) * n, a * n:(a + 1) * n].tocsr() for a in (0, 1)]
    A1 = [J1s[a * n1:(a + 1) * n1, a * n1:(a + 1) * n1].tocsr() for a in (0, 1)]
    _compare_with_numpy_cycle(pre, A, A1, P, bc0, bc1, n, n1)


@pytest.mark.gpu
def test_one_plane_levels_match_the_numpy_cycle(newton_system, monkeypatch):
    '''The optional one-plane levels (flow_pmg_pack1: the mean of the two
    blocks as a packed 4-byte stream, identity rows by flag) against the same
    restatement on the operators `_one_plane` builds.'''
    from flow_amd import device
    from flow_amd.fem import pmg as fpmg
    prob, infos, pre0, J, J1 = newton_system
    lay = prob.W.layout
    n, n1 = lay.N, pre0.lay1.N
    monkeypatch.setattr(fpmg, 'ONE_PLANE', True)
    pre = fpmg.Pmg(prob.W)
    assert pre.fine.struct.packed and pre.coarse.struct.packed
    bc0 = device.to_host(pre0._keep['bc_fine']).numpy().astype(bool)
    bc1 = device.to_host(pre0._keep['bc_coarse']).numpy().astype(bool)
    pre.set_bcs(numpy.nonzero(bc0)[0].astype(numpy.int32))
    pre.refactor(J, J1)
    # the identity rows it found are the Dirichlet dofs
    for lvl, m in ((pre.fine, bc0), (pre.coarse, bc1)):
        assert numpy.array_equal(
            device.to_host(lvl._packed[1]).numpy().astype(bool), m)
    Js, J1s = J.to_scipy().tocsr(), J1.to_scipy().tocsr()
    P = _prolongation(lay)[0]
    _compare_with_numpy_cycle(pre, _one_plane(Js, n), _one_plane(J1s, n1), P,
                              bc0, bc1, n, n1)
    # the spectral radius the power method sees is this operator's
    for lvl, Ms, lam, nn in ((pre.fine, Js, pre.lam[0], n),
                             (pre.coarse, J1s, pre.lam[1], n1)):
        want = 0.0
        for B in _one_plane(Ms, nn):
            DB = sp.diags(1.0 / B.diagonal()).dot(B)
            ev = spla.eigs(DB, k=1, which='LM', return_eigenvectors=False,
                           tol=1e-4)
            want = max(want, abs(ev[0]))
        assert 0.93 * want < lam <= 1.001 * want, (lam, want)


@pytest.mark.gpu
def test_int32_columns_match_the_numpy_cycle_and_the_16_bit_offsets(
        newton_system, monkeypatch):
    '''The fallback format of the two-plane levels (int32 columns: what a level
    gets when a tile's columns span 65536 or more) against the numpy cycle,
    and against the default format (16-bit offsets from the tile's lowest
    column) bit for bit: the two encode the same columns and the same fp16
    values and go through the one tile routine (fp16_tile_row_sum), so the
    power iterations find the same intervals and the cycles the same z.'''
    from flow_amd import device
    from flow_amd.fem import pmg as fpmg
    prob, infos, pre0, J, J1 = newton_system
    lay = prob.W.layout
    n, n1 = lay.N, pre0.lay1.N
    bc0 = device.to_host(pre0._keep['bc_fine']).numpy().astype(bool)
    bc1 = device.to_host(pre0._keep['bc_coarse']).numpy().astype(bool)

    def fresh(cols16):
        monkeypatch.setattr(fpmg, 'COLS16', cols16)
        pre = fpmg.Pmg(prob.W)
        for lvl in (pre.fine, pre.coarse):
            assert bool(lvl.struct.cols16) == cols16 and not lvl.struct.packed
        pre.set_bcs(numpy.nonzero(bc0)[0].astype(numpy.int32))
        return pre.refactor(J, J1)
    pre32, pre16 = fresh(False), fresh(True)
    assert pre32.lam == pre16.lam
    Js, J1s = J.to_scipy().tocsr(), J1.to_scipy().tocsr()
    P = _prolongation(lay)[0]
    A = [Js[a * n:(a + 1) * n, a * n:(a + 1) * n].tocsr() for a in (0, 1)]
    A1 = [J1s[a * n1:(a + 1) * n1, a * n1:(a + 1) * n1].tocsr() for a in (0, 1)]
    _compare_with_numpy_cycle(pre32, A, A1, P, bc0, bc1, n, n1)
    r = device.to_device(numpy.random.RandomState(6).standard_normal(2 * n))
    z32 = device.to_host(pre32.apply(r, device.zeros(2 * n))).numpy()
    z16 = device.to_host(pre16.apply(r, device.zeros(2 * n))).numpy()
    assert numpy.isfinite(z32).all() and numpy.array_equal(z32, z16)


def _compare_with_numpy_cycle(pre, A, A1, P, bc0, bc1, n, n1):
    from flow_amd import device
    rng = numpy.random.RandomState(4)
    for trial in range(2):
        r = rng.standard_normal(2 * n)
        if trial == 1:
            r[bc0] = 0.0          # what the Newton systems hand it
        z = device.zeros(2 * n)
        pre.apply(device.to_device(r), z)
        got = device.to_host(z).numpy()
        ref = numpy.concatenate([
            _cycle(pre, A[a], A1[a], P, bc0[a * n:(a + 1) * n],
                   bc1[a * n1:(a + 1) * n1], r[a * n:(a + 1) * n])
            for a in (0, 1)])
        # fp16 matrix entries (relative 5e-4 each) and fp32 vectors inside
        assert cases.rel_l2(got, ref) < 2e-3, trial
        assert numpy.array_equal(got[bc0], r[bc0])


@pytest.mark.gpu
def test_spectral_radius_estimate(newton_system):
    prob, infos, pre, J, J1 = newton_system
    for lvl, M, lam in ((pre.fine, J, pre.lam[0]), (pre.coarse, J1, pre.lam[1])):
        Ms = M.to_scipy().tocsr()
        n = lvl.lay.N
        want = 0.0
        for a in (0, 1):
            B = Ms[a * n:(a + 1) * n, a * n:(a + 1) * n].tocsr()
            DB = sp.diags(1.0 / B.diagonal()).dot(B)
            ev = spla.eigs(DB, k=1, which='LM', return_eigenvectors=False,
                           tol=1e-4)
            want = max(want, abs(ev[0]))
        # the power method from a fixed start after 32 steps: a lower bound
        # within a few per cent (the interval adds 10 % on top)
        assert 0.93 * want < lam <= 1.001 * want, (lam, want)
        assert lvl.struct.lam_max >= 0.99 * want


@pytest.mark.gpu
def test_gmres_with_the_cycle_against_direct_solve_and_ilu(newton_system):
    from flow_amd import device
    from flow_amd.fem import ilu, ops
    prob, infos, pre, J, J1 = newton_system
    lay = prob.W.layout
    n = lay.N
    Js = J.to_scipy().tocsc()
    rng = numpy.random.RandomState(8)
    b = rng.standard_normal(2 * n)
    ref = spla.splu(Js).solve(b)
    counts = {}
    for name, kw in (('pmg', dict(pmg=pre)),
                     ('ilu0', dict(ilu=ilu.Ilu0(J, packed=True,
                                                single_vector=True)))):
        x = device.zeros(2 * n)
        info = ops.krylov_solve('gmres', J, device.to_device(b), x, rtol=1e-10,
                                maxit=400, restart=10, x_is_zero=True,
                                dinv=None, **kw)
        assert cases.rel_l2(device.to_host(x).numpy(), ref) < 1e-8, (name, info)
        counts[name] = info.iterations
    print('GMRES(10) applications to 1e-10:', counts)
    assert counts['pmg'] < counts['ilu0'], counts
    # the steps of the fixture converged with it, one Newton iteration each
    for i in infos:
        assert len(i['newton_residuals']) >= 2
        assert i['newton_residuals'][-1] < 1e-10
