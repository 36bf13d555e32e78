# -*- coding: utf-8 -*-
'''
UFL-style integrands of fields: what the reference's drivers write around a
step -- `assemble(p*dx(mesh))`, `project(sqrt(ux**2 + uy**2), Q)`,
`project(rho(theta)*g*y, P)` with `y = SpatialCoordinate(mesh)[1]` -- built
with operator overloading and expanded on the host into SCALAR trees (tensors
are rank <= 2 and exist only here).  Each tree is compiled to a small register
program (include/flow_hip.h, flow_form) that one HIP kernel family runs at the
quadrature points of every cell (flow_amd/csrc/form_kernels.hip); the device
calls are `ops.assemble` and `ops.project`.  Building and compiling trees is
host-only and needs no library.

Operands: Function (scalar or 2-vector, P1 or P2; `u[i]`, `u.split()`
copies), Constant, plain numbers, Expression (through its P_k cell lattice,
k <= 5, as `as_cell_coefficient` interpolates it: dolfin's "interpolate into
P_degree"), SpatialCoordinate(mesh), as_vector([...]).
Operators: + - * / unary -, ** (a non-negative integer exponent becomes
repeated multiplies, a negative one their reciprocal, any other exponent
pow), abs(), sqrt exp ln sin cos, dot inner grad div curl, f.dx(i).  In 2-D
curl of a vector is the scalar dv/dx - du/dy (of a scalar s: (ds/dy, -ds/dx)).

Quadrature degree: UFL's estimation rules, applied to the tensor expression
  Function / Expression   its degree        SpatialCoordinate  1
  Constant, number        0                 a + b, a - b       max
  a * b, dot, inner       sum               a / b              deg a + deg b
  a**n (int n >= 0)       n deg a           other powers       deg a + 2
  sqrt exp ln sin cos     deg + 2           abs, unary -       unchanged
  grad div curl .dx       max(deg - 1, 0)   as_vector, [i]     max / unchanged
`project(f, V)` adds the test space's degree; `dx(metadata={'quadrature_degree':
q})` or `form_compiler_parameters={'quadrature_degree': q}` replaces the
estimate.  q <= 30.  The rules are reference.triangle_rule(q) (collapsed
Gauss-Jacobi, exact for total degree q), not FFC's point sets: for integrands
that are polynomials within the degree the results are dolfin's; otherwise
they differ from dolfin's by quadrature error.

Exterior facets: `f*ds` integrates over the boundary edges of the mesh, with
dolfin-2017's spellings -- ds(mesh), ds(domain=mesh), ds(1),
ds(subdomain_id=1), ds(metadata={...}), ds(degree=q) and
Measure('ds', domain=mesh, subdomain_data=markers) then ds(k), where markers
is a MeshFunction('size_t', mesh, 1) (or FacetFunction) filled by
SubDomain.mark.  FacetNormal(mesh) (the outward unit normal, degree 0) is
legal only in ds integrands.  The rule is reference.line_rule(q) on each
edge (Gauss-Legendre, exact for degree q).  Rank-0 forms add and subtract:
assemble(f*dx + g*ds(1) - h*ds(2)) sums the parts in the order written.
No facet integrals on strips.

Interior facets are OFF by default, as they always were (NotImplementedError);
`interior_facets(True)` switches them on like facet_arguments.  Then `f*dS`,
dS(mesh), dS(k) and Measure('dS', domain=mesh, subdomain_data=markers)(k) are
forms of integral_type 'interior_facet' over the edges with two cells (those
whose marker equals k), f('+') / f('-') restricts any scalar, vector or
tensor expression to a side -- pushed down to the leaves at once: ('side',
leaf, s) --, jump(f) = f('+') - f('-'), jump(f, n) = f('+')*n('+') +
f('-')*n('-') (scalar f: a vector) or the same with dot (vector f: a scalar),
avg(f) = (f('+') + f('-'))/2, FacetArea(mesh) the facet's length (degree 0).
'+' is the cell with the SMALLER cell index.  UFL's apply_restrictions rules:
values of Functions, SpatialCoordinate, Constants, numbers and FacetArea may
stand unrestricted under dS (continuous: evaluated on '+'); gradients,
FacetNormal, CellVolume, Circumradius and CellDiameter must be restricted
(ValueError naming the operand); a restriction under dx / ds, or of a
restricted expression, is a ValueError.  Every (Function, component, side) is
one of the MAX_FIELDS field slots of a program: u('+') and u('-') are two.
Refused (NotImplementedError, switch on or off): test and trial functions
under dS (restricted arguments need twice the coefficient slots and, for rank
2, a sparsity pattern wider than the space's), Expression operands and the
SUPG tau under dS (their tables are indexed by the rule's row of one cell),
FacetArea under dx / ds, derivative of a dS part, strips.  The degree is
estimated, and replaced by dS(degree=q) or form_compiler_parameters, as for
ds.  ops.assemble (a float; signed sums mix dx, ds and dS),
ops.interior_facet_integrals and ops.cell_indicator are the device calls.

Arguments: `v = TestFunction(V)`, `u = TrialFunction(V)` on a scalar P1 / P2
space are operands like any other (degree = the space's), so `grad`, `dot`,
`inner`, `.dx(i)`, `v/c` and products with coefficients work unchanged.  A
form's rank is the number of distinct arguments in it: `assemble` gives a float
(0), a Vector (1) or a Matrix (2); `lhs` / `rhs` / `system` split a signed sum
of forms, `a == L` is an Equation for `solve`.  On the host the integrand of a
rank-2 form is rewritten by linearity as sum_(b,a) c[b][a] D_a u D_b v, of a
rank-1 form as sum_b c[b] D_b v (D_0 value, D_1 d/dx, D_2 d/dy;
`extract_arguments`): + - and unary - distribute, * multiplies the two sides'
tables, / needs an argument-free denominator, anything else applied to an
argument is a ValueError.  The coefficients c are argument-free scalar trees;
they compile to one Program with one output slot per term (3 b + a, or b).
`form_compiler_parameters={'quadrature_rule': 'vertex'}` integrates with the
cell vertices and weights |T|/3 (the lumped mass matrix of u*v*dx).
Arguments under ds (Neumann, Robin and Nitsche terms) are OFF by default, as
they always were (NotImplementedError); `facet_arguments(True)` switches them
on for the process (it returns the previous setting; `with
facet_arguments(True): ...` restores it on exit).  Then `g*v*ds(2)`,
`h*u*v*ds(1)`, `-dot(grad(u), n)*v*ds` are forms of integral_type
'exterior_facet' and rank 1 or 2; FacetNormal stays legal there, all the dofs
of the owning cell take part (grad(u) of the off-edge basis function is not
zero on the edge), and rank, arguments(), argument_table(), lhs / rhs / system
and is_symmetric_table work on them as on dx parts -- h*(u - u_inf)*v*ds
splits into its Robin pair.  They are assembled by one lane per (facet, local
test dof) and a gather over the facet contribution map (ops.facet_map).
Refused there: 'quadrature_rule': 'vertex' (ValueError: the vertex rule is a
rule of cells) and strips (NotImplementedError).  The limit on field
components is that of every program (MAX_FIELDS): the kernel's instance for
six fields still runs without scratch memory or spills.
Arguments on a vector space (2x2-block forms: elasticity inner(sigma(u),
eps(v))*dx, grad-div, the vector Laplacian, a Brinkman operator) are OFF by
default too, as they always were (NotImplementedError);
`vector_arguments(True)` switches them on like facet_arguments.  Then
TestFunction(W) / TrialFunction(W) of a P1 / P2 VectorFunctionSpace is a
2-vector whose components are leaves ('arg', number, d, W, comp) -- scalar
arguments keep their 4-tuple --, so u[i], grad(u) (2x2), div, curl, dot,
inner, as_vector, conditional and the tensor helpers sym(A), tr(A),
transpose(A) / A.T, Identity(2), outer(a, b) (rank-2 FormExprs, with or without
arguments; degrees by UFL's rules: sym tr transpose unchanged, Identity 0, outer
the sum) work through the tensor machinery above.  extract_arguments keys
become ((b, r), (a, s)), r the test and s the trial component; argument_table
gives table[r][s] (rank 2) or table[r] (rank 1), each the table of a SCALAR
form or None for a block without a term (callers tell by the space's dim);
is_symmetric_table asks c[r][s][b][a] == c[s][r][a][b]; every present block
compiles with argument_programs to the programs of a scalar form
(block_items).  assemble gives a Matrix of kind 2 (four value planes over the
scalar pattern, plane 2 r + s) or a Vector of 2N, component-major
(flow_form_block_matrix / flow_form_block_vector); ds parts need both
switches.  Refused there (NotImplementedError): W.sub(i) as an argument
space, Eigenmodes, strips, and -- OFF by default like the arguments
themselves -- derivative() with respect to a vector Function and solve(F ==
0): `vector_derivatives(True)` switches those on (below).
Arguments on a Taylor-Hood space WP = VectorElement(P_kv) * FiniteElement(P_kp),
kv, kp in {1, 2}, are OFF by default too (NotImplementedError);
`mixed_arguments(True)` switches them on (it implies no other switch):
TestFunctions(WP) / TrialFunctions(WP) give (vector, scalar) pairs whose leaves
are ('arg', number, d, WP, comp), comp 0, 1 (velocity), 2 (pressure);
argument_table gives a MixedTable of 3 x 3 (rank 1: 3) scalar tables whose
velocity() corner is the BlockTable of a vector form; is_symmetric_form judges
symmetry over all parts of a sum; Function(WP), split(w), w.split(), w.sub(i)
(function.py); assembly and solve: fem/mixed.py.
Not supported (NotImplementedError): arguments on other mixed spaces, a mixed
argument together with an argument of another space, test
and trial functions of different spaces (a vector test function with a scalar
trial function included), arguments under dS, action / adjoint.  lhs / rhs
also split ONE integrand that holds terms of
both ranks, (source - dot(conv, grad(u))) * tau * dot(conv, grad(v)) * dx, by
linearity, as UFL does; assembling such an integrand unsplit stays a
ValueError.

Derivatives: `derivative(F, u, du=None)` is the Gateaux derivative of a form
(or signed sum) of rank 0 or 1 with respect to a scalar P1 / P2 Function u,
taken on the scalar trees like s_diff's spatial chain rule (s_gateaux): the
leaf ('field', u, 0, d) becomes ('arg', k, d, V), V = u.function_space(), k =
the number of arguments F already has (a functional gives a form in the test
function, a residual one in the trial function); every other leaf is zero;
add sub neg mul div powi pow sqrt exp ln sin cos abs follow the usual rules
(abs(a): a/abs(a) da), zeros fold away, and the new argument only ever lands
in numerators and products, so the result passes extract_arguments as it is.
It works part by part (sign, measure, metadata and mesh are kept; parts that
do not depend on u vanish), twice on an energy functional it gives the
bilinear form.  A derived part keeps the quadrature degree of the part it
came from (unless metadata fixes one): for integrands polynomial in u that IS
UFL's estimate -- replacing a factor u by du of the same space leaves the sum
of degrees unchanged --, for the others it differs from dolfin's by
quadrature error, like the estimates above.  ds parts are derived like dx
parts (a rank-0 ds functional gives a rank-1 ds form, a rank-1 ds residual
part a rank-2 ds part) and keep their subdomain id and subdomain data too
-- with facet_arguments(True); without it a ds part that holds u is refused.
Refused: a rank-2 form (the result would be a rank-3 form), u on a vector,
component or mixed space, a form that does not depend on u, u of another
space than the form's arguments.  With `vector_derivatives(True)` (a process
switch like vector_arguments, which it needs as well: alone it refuses with a
message that names that switch) u may live on a P1 / P2 VectorFunctionSpace
W: the leaf ('field', u, i, d) becomes ('arg', k, d, W, i), every other rule,
the parts, signs, metadata, subdomain data, derived_from and the degree rule
are the scalar ones; du, if given, is the TestFunction(W) / TrialFunction(W)
of the right number; a functional gives a rank-1 form on W, a residual its
2x2-block Jacobian, an energy twice the bilinear form.  Still refused: u on
W.sub(i) or a mixed space, a rank-2 F, arguments of another space than u's (a
scalar Function in a form on W included), a form that does not depend on u.
solve(F == 0) on W is then the block Newton of ops.newton_solve
(flow_form_block_newton).  `F == 0` is the
Equation of the nonlinear solve(F == 0, u, bcs, J=...) (ops.solve: Newton);
a form of any rank compared with the number 0 gives one (solve refuses what
is not a residual), any other number is a ValueError.
newton_program() compiles the tables of J and F into one Program (slots
3 b + a and 9 + b of 12) that computes the subtrees the two share once.

Branches, clips and cell geometry (UFL's spellings):
  operand / operator                   degree            d/dx and Gateaux
  conditional(c, t, f)                 max(deg t, deg f) conditional(c, t', f')
  max_value(a, b)                      max               conditional(gt(a, b), a', b')
  min_value(a, b)                      max               conditional(lt(a, b), a', b')
  sign(a)                              deg a             0
  tanh(a)                              deg a + 2         (1 - tanh(a)^2) a'
  CellVolume Circumradius CellDiameter 0                 0
  stabilization.supg(...) (SUPG tau)   1                 Gateaux 0; d/dx refused
Conditions are lt le gt ge eq ne of two scalars (also a < b, a <= b, ...) and
And Or Not of conditions.  A condition is NOT a scalar operand: arithmetic with
one is a TypeError, a number in its place too; it is never differentiated and
does not count in the degree.  t and f are scalars or tensors of one shape
(component by component).  conditional is a SELECT: both branches are
computed and the value of the untaken one never reaches the result, so
conditional(gt(Pe, 1e-5), (1/tanh(Pe) - 1/Pe)/Pe, 1/3 - Pe**2/45) is 1/3 at
Pe == 0 although the other branch is inf - inf there.  On the device a
condition is 1.0 or 0.0 (opcodes lt le eq ne; gt and ge swap their operands;
And is the product, Or the larger, Not 1 - c) and `select` is R[dst] = R[a]
!= 0 ? R[b] : R[dst]; Program.need counts its three live values.  The
geometry operands are cell-wise constants that carry their mesh (the owning
cell under ds and at points): CellVolume |T|, Circumradius abc / (4 |T|),
CellDiameter the largest vertex distance, computed on the device from the
vertex coordinates a lane holds.  An argument may sit in the BRANCHES of a
conditional: extract_arguments distributes it over the two branches' tables,
c[b][a] = conditional(cond, c_t, c_f) with zero where a branch lacks the
term; an argument in a condition or under max_value / min_value / sign /
tanh is the "not linear" ValueError.  The SUPG tau is the values at the three
vertices of each cell, linear inside, discontinuous across cells: an 'expr'
leaf whose lattice flow_supg_tau computes at every launch from the convection
field as it then is; legal under dx and ds, not at points.  sinh, cosh and
atan are not provided: each needs an inlined routine of its own in the
interpreter (tanh shares the one exp), and the interpreter's instances are at
their register limits.  Programs with an opcode from 19 up run on
instances of the kernels compiled for them; every other program launches the
instances it always did.  compile_trees() computes subtrees that repeat
within an integrand once where the plain program exceeds a limit of flow_form.
'''
import numbers

from .function import Function, Constant, Expression

MAX_QUADRATURE_DEGREE = 30
# include/flow_hip.h
MAX_PROGRAM = 64
REGISTERS = 8
MAX_CONSTANTS = 32
MAX_FIELDS = 6
MAX_EXPRESSIONS = 4
NEWTON_SLOTS = 12       # 9 of the Jacobian's table, 3 of the residual's
OPS = {name: i for i, name in enumerate((
    'const', 'coord', 'field', 'expr', 'mov', 'add', 'sub', 'mul', 'div', 'pow',
    'neg', 'abs', 'sqrt', 'exp', 'ln', 'sin', 'cos', 'out', 'normal',
    # 19 up: conditions (1.0 | 0.0), the select, clips, tanh, cell geometry
    'lt', 'le', 'eq', 'ne', 'select', 'min', 'max', 'sign', 'tanh', 'cell',
    # 29: the length of the facet (interior-facet programs only)
    'facet_len'))}
# interior-facet programs: the side bit of the leaf instructions ('+' clear,
# '-' set) -- FIELD in b (beside the derivative 0..2), NORMAL in a (beside the
# component 0..1), CELL in a (beside the quantity 0..2); include/flow_hip.h
SIDE_BIT = {'field': 4, 'normal': 2, 'cell': 4}
UNARY = ('neg', 'abs', 'sqrt', 'exp', 'ln', 'sin', 'cos')
BINARY = ('add', 'sub', 'mul', 'div', 'pow')
# the extended vocabulary: nodes like the above that no argument may sit under
UNARY_EXT = ('sign', 'tanh')
BINARY_EXT = ('max', 'min')
COMPARE = ('lt', 'le', 'gt', 'ge', 'eq', 'ne')
# every node with subtrees: (op, a[, b]), ('powi', a, n), ('cond', c, t, f)
NONLEAF = UNARY + BINARY + ('powi',) + UNARY_EXT + BINARY_EXT + COMPARE \
    + ('cond',)
CELL_QUANTITIES = ('volume', 'circumradius', 'diameter')


# -- scalar trees --------------------------------------------------------------
# ('num', v) ('const', Constant, i) ('x', d) ('field', Function, i, d)
# (d = 0 value, 1 d/dx, 2 d/dy) ('expr', Expression, i) ('n', d) (component
# d of the outward unit normal, ds only) ('arg', number, d, V) (number 0 the
# test, 1 the trial function of the space V; d as for fields; of a vector
# space: ('arg', number, d, V, comp), component comp) ('powi', a, n)
# and (op, a[, b]) for the UNARY / BINARY ops; ('reg', r) (register r of the
# program, holding a subtree computed up front: newton_program only);
# ('cell', mesh, k) (k = 0 |T|, 1 the circumradius, 2 the diameter of the cell);
# (op, a[, b]) for UNARY_EXT / BINARY_EXT; (op, a, b) for COMPARE, worth 1.0
# or 0.0 (And = mul, Or = max, Not = 1 - c of those); ('cond', c, t, f), t
# where c != 0 and f elsewhere -- a select, the untaken value is not read.
# ('side', leaf, s): the leaf (a field, n, cell or arg leaf) restricted to the
# '+' (s = 0) or '-' (s = 1) cell of an interior facet -- a leaf itself: the
# restriction is pushed down to the leaves when it is applied; ('farea',
# mesh): the length of the facet (dS only).
# Objects inside compare by identity.
ZERO = ('num', 0.0)
ONE = ('num', 1.0)


def _is_num(n, v=None):
    return n[0] == 'num' and (v is None or n[1] == v)


def s_add(a, b):
    if _is_num(a, 0.0):
        return b
    if _is_num(b, 0.0):
        return a
    return ('add', a, b)


def s_sub(a, b):
    if _is_num(b, 0.0):
        return a
    if _is_num(a, 0.0):
        return s_neg(b)
    return ('sub', a, b)


def s_mul(a, b):
    if _is_num(a, 0.0) or _is_num(b, 0.0):
        return ZERO
    if _is_num(a, 1.0):
        return b
    if _is_num(b, 1.0):
        return a
    return ('mul', a, b)


def s_div(a, b):
    if _is_num(a, 0.0):
        return ZERO
    if _is_num(b, 1.0):
        return a
    return ('div', a, b)


def s_neg(a):
    if _is_num(a):
        return ('num', -a[1])
    return ('neg', a)


def s_powi(a, n):
    if n < 0:
        return s_div(ONE, s_powi(a, -n))
    if n == 0:
        return ONE
    if n == 1:
        return a
    return ('powi', a, n)


def s_cond(c, t, f):
    '''t where c holds, f elsewhere; equal branches need no condition.'''
    if t == f:
        return t
    return ('cond', c, t, f)


def s_diff(n, d):
    '''d n / d x_d (d = 0, 1), by the chain rule.'''
    k = n[0]
    if k in ('num', 'const', 'n', 'cell', 'sign', 'farea'):
        # (the normal: constant on a facet; cell geometry: on a cell)
        return ZERO
    if k == 'side':                     # (grad(u('+')) is grad(u)('+'))
        inner_d = s_diff(n[1], d)
        return inner_d if _is_num(inner_d) else ('side', inner_d, n[2])
    if k == 'cond':                     # (the condition is not differentiated)
        return s_cond(n[1], s_diff(n[2], d), s_diff(n[3], d))
    if k in ('max', 'min'):
        return s_cond(('gt' if k == 'max' else 'lt', n[1], n[2]),
                      s_diff(n[1], d), s_diff(n[2], d))
    if k == 'x':
        return ONE if n[1] == d else ZERO
    if k == 'field':
        if n[3] != 0:
            raise NotImplementedError('second derivatives of a field')
        return ('field', n[1], n[2], d + 1)
    if k == 'expr':
        if _has_lattice(n[1]):
            raise NotImplementedError(
                'spatial derivatives of the SUPG tau (a cell-wise linear, '
                'discontinuous coefficient given by its vertex values) are '
                'not supported')
        raise NotImplementedError(
            'derivatives of an Expression: interpolate it into a Function')
    if k == 'arg':
        if n[2] != 0:
            raise NotImplementedError('second derivatives of a test or trial '
                                      'function')
        # (a component of a vector argument keeps its fifth entry)
        return n[:2] + (d + 1,) + n[3:]
    if k == 'add':
        return s_add(s_diff(n[1], d), s_diff(n[2], d))
    if k == 'sub':
        return s_sub(s_diff(n[1], d), s_diff(n[2], d))
    if k == 'neg':
        return s_neg(s_diff(n[1], d))
    a = n[1]
    da = s_diff(a, d)
    if k == 'mul':
        return s_add(s_mul(da, n[2]), s_mul(a, s_diff(n[2], d)))
    if k == 'div':
        b = n[2]
        return s_div(s_sub(s_mul(da, b), s_mul(a, s_diff(b, d))), s_powi(b, 2))
    if k == 'powi':
        return s_mul(s_mul(('num', float(n[2])), s_powi(a, n[2] - 1)), da)
    if k == 'pow':
        b = n[2]
        return s_mul(n, s_add(s_mul(s_diff(b, d), ('ln', a)),
                              s_div(s_mul(b, da), a)))
    if k == 'sqrt':
        return s_div(da, s_mul(('num', 2.0), n))
    if k == 'exp':
        return s_mul(n, da)
    if k == 'ln':
        return s_div(da, a)
    if k == 'sin':
        return s_mul(('cos', a), da)
    if k == 'cos':
        return s_neg(s_mul(('sin', a), da))
    if k == 'tanh':
        return s_mul(s_sub(ONE, s_powi(n, 2)), da)
    raise NotImplementedError('derivative of %s' % k)


def s_gateaux(n, u, k, V):
    '''d n / d u in the direction of argument number k of V = the space of the
    Function u: s_diff's chain rule with another leaf rule.  u scalar:
    ('field', u, 0, d) becomes ('arg', k, d, V); u on a vector space: ('field',
    u, i, d) becomes ('arg', k, d, V, i), component i of the vector argument.'''
    op = n[0]
    if op == 'field':
        if is_mixed_space(V):
            # (u a Function of a Taylor-Hood space, mixed_derivatives: its
            # fields are the views u.split() makes afresh at every call, known
            # by their owner; the leaves are those of TrialFunctions(V))
            own = getattr(n[1], 'mixed_owner', None)
            if own is None or own[0] is not u:
                return ZERO
            return ('arg', k, n[3], V, n[2] if own[1] == 0 else 2)
        if n[1] is u and V.dim == 2:
            return ('arg', k, n[3], V, n[2])
        if n[1] is u and n[2] == 0:
            return ('arg', k, n[3], V)
        return ZERO
    if op in ('num', 'const', 'x', 'expr', 'n', 'arg', 'cell', 'sign'):
        return ZERO
    if op == 'cond':
        return s_cond(n[1], s_gateaux(n[2], u, k, V), s_gateaux(n[3], u, k, V))
    if op in ('max', 'min'):
        return s_cond(('gt' if op == 'max' else 'lt', n[1], n[2]),
                      s_gateaux(n[1], u, k, V), s_gateaux(n[2], u, k, V))
    a = n[1]
    da = s_gateaux(a, u, k, V)
    if op == 'neg':
        return s_neg(da)
    if op == 'tanh':
        return s_mul(s_sub(ONE, s_powi(n, 2)), da)
    if op == 'powi':
        return s_mul(s_mul(('num', float(n[2])), s_powi(a, n[2] - 1)), da)
    if op == 'sqrt':
        return s_div(da, s_mul(('num', 2.0), n))
    if op == 'exp':
        return s_mul(n, da)
    if op == 'ln':
        return s_div(da, a)
    if op == 'sin':
        return s_mul(('cos', a), da)
    if op == 'cos':
        return s_neg(s_mul(('sin', a), da))
    if op == 'abs':
        return s_mul(s_div(a, n), da)
    if op not in BINARY:
        raise NotImplementedError('derivative of %s' % op)
    b = n[2]
    db = s_gateaux(b, u, k, V)
    if op == 'add':
        return s_add(da, db)
    if op == 'sub':
        return s_sub(da, db)
    if op == 'mul':
        return s_add(s_mul(da, b), s_mul(a, db))
    if op == 'div':
        # (da / b - a db / b^2: the argument stays in the numerators)
        return s_sub(s_div(da, b), s_div(s_mul(a, db), s_powi(b, 2)))
    # pow
    return s_mul(n, s_add(s_mul(db, ('ln', a)), s_div(s_mul(b, da), a)))


# -- tensors of scalar trees -----------------------------------------------------
def _map(f, c, shape):
    if len(shape) == 0:
        return f(c)
    return [_map(f, ci, shape[1:]) for ci in c]


def _map2(f, a, b, shape):
    if len(shape) == 0:
        return f(a, b)
    return [_map2(f, ai, bi, shape[1:]) for ai, bi in zip(a, b)]


def _flat(c, shape):
    if len(shape) == 0:
        return [c]
    return [x for ci in c for x in _flat(ci, shape[1:])]


def _join_mesh(a, b):
    if a is not None and b is not None and a is not b:
        raise ValueError('the expression combines fields of two different '
                         'meshes')
    return a if a is not None else b


def _join(a, b):
    '''The mesh of a combination of two FormExprs.  Fields of two meshes
    are a ValueError (_join_mesh); a test and a trial function of two meshes
    are out of scope like those of two spaces: NotImplementedError.'''
    if a.mesh is not None and b.mesh is not None and a.mesh is not b.mesh \
            and all(any(has_leaf(t, 'arg') for t in e.scalar_trees())
                    for e in (a, b)):
        raise NotImplementedError(
            'test and trial functions on different meshes')
    return _join_mesh(a.mesh, b.mesh)


_FORM_OPERANDS = ()     # filled below


class FormExpr(object):
    '''A tensor (rank <= 2, 2-D) of scalar trees with its estimated degree.
    No __eq__ / __hash__: expressions, like the Functions inside them, compare
    and hash by identity.'''
    __array_ufunc__ = None          # numpy scalars defer to the operators below

    def __init__(self, comps, shape, deg, mesh=None):
        if len(shape) > 2:
            raise ValueError('tensors of rank %d: at most rank 2 is supported'
                             % len(shape))
        self.comps = comps
        self.shape = tuple(shape)
        self.deg = int(deg)
        self.mesh = mesh

    def rank(self):
        return len(self.shape)

    def scalar_trees(self):
        return _flat(self.comps, self.shape)

    # -- arithmetic
    def __add__(self, other):
        return _binary('add', self, other)

    def __radd__(self, other):
        return _binary('add', other, self)

    def __sub__(self, other):
        return _binary('sub', self, other)

    def __rsub__(self, other):
        return _binary('sub', other, self)

    def __mul__(self, other):
        if isinstance(other, Measure):
            return other.__rmul__(self)
        return _binary('mul', self, other)

    def __rmul__(self, other):
        return _binary('mul', other, self)

    def __truediv__(self, other):
        return _binary('div', self, other)

    def __rtruediv__(self, other):
        return _binary('div', other, self)

    __div__ = __truediv__
    __rdiv__ = __rtruediv__

    def __pow__(self, other):
        return _power(self, other)

    def __rpow__(self, other):
        return _power(other, self)

    def __neg__(self):
        return FormExpr(_map(s_neg, self.comps, self.shape), self.shape,
                        self.deg, self.mesh)

    def __pos__(self):
        return self

    def __abs__(self):
        return _function('abs', self)

    # (UFL: a < b is lt(a, b); == and != stay identity, use eq() and ne())
    def __lt__(self, other):
        return lt(self, other)

    def __le__(self, other):
        return le(self, other)

    def __gt__(self, other):
        return gt(self, other)

    def __ge__(self, other):
        return ge(self, other)

    def __getitem__(self, idx):
        if not isinstance(idx, tuple):
            idx = (idx,)
        if len(idx) > len(self.shape):
            raise ValueError('index %r of a tensor of shape %r'
                             % (idx, self.shape))
        c = self.comps
        for i in idx:
            if not isinstance(i, numbers.Integral):
                raise TypeError('component indices are integers')
            if not 0 <= i < 2:
                raise IndexError(i)
            c = c[i]
        return FormExpr(c, self.shape[len(idx):], self.deg, self.mesh)

    @property
    def T(self):
        return transpose(self)

    def __call__(self, side):
        '''f('+') / f('-'): the restriction to a side of an interior facet
        (interior_facets(True)); see restricted().'''
        return restricted(self, side)

    def dx(self, i):
        if i not in (0, 1):
            raise IndexError('dx(%r): the mesh is 2-D' % (i,))
        return FormExpr(_map(lambda n: s_diff(n, i), self.comps, self.shape),
                        self.shape, max(self.deg - 1, 0), self.mesh)


def as_form(obj):
    '''The FormExpr of an operand; TypeError if it is none.'''
    if isinstance(obj, FormExpr):
        return obj
    if isinstance(obj, bool):
        raise TypeError('not a form operand: %r' % (obj,))
    if isinstance(obj, Condition):
        raise TypeError(Condition.REFUSAL)
    if isinstance(obj, numbers.Real):
        return FormExpr(('num', float(obj)), (), 0)
    if isinstance(obj, Function):
        V = obj.function_space()
        if V.degree not in (1, 2):
            raise ValueError('fields of degree 1 or 2 only')
        if V.dim == 1:
            return FormExpr(('field', obj, 0, 0), (), V.degree, V.mesh())
        return FormExpr([('field', obj, i, 0) for i in range(V.dim)], (V.dim,),
                        V.degree, V.mesh())
    if isinstance(obj, Constant):
        vals = obj.values()
        if len(vals) == 1:
            return FormExpr(('const', obj, 0), (), 0)
        if len(vals) != 2:
            raise ValueError('Constant with %d components' % len(vals))
        return FormExpr([('const', obj, i) for i in range(2)], (2,), 0)
    if isinstance(obj, Expression):
        k = int(obj.degree)
        if not 0 <= k <= 5:
            raise ValueError('Expression degree must be <= 5 (got %d)' % k)
        dim = obj.value_dim()
        if dim == 1:
            return FormExpr(('expr', obj, 0), (), k)
        if dim != 2:
            raise ValueError('Expression with %d components' % dim)
        return FormExpr([('expr', obj, i) for i in range(2)], (2,), k)
    if _has_lattice(obj):
        return FormExpr(('expr', obj, 0), (), int(obj.degree), obj.mesh)
    raise TypeError('not a form operand: %r' % (type(obj),))


def _has_lattice(obj):
    '''A scalar coefficient that computes its own P_degree cell lattice on
    the device (stabilization.SupgTau: the values at the cell vertices, linear
    inside a cell, discontinuous across cells): an 'expr' leaf that carries
    its mesh; ops._form_struct calls obj.form_lattice(mesh) at every launch.'''
    return hasattr(obj, 'form_lattice') and hasattr(obj, 'degree')


def is_form_operand(obj):
    return isinstance(obj, (FormExpr, Function, Constant, Expression, Measure,
                            Condition, _InteriorFacets)) or _has_lattice(obj)


def _binary(op, a, b):
    try:
        a = as_form(a)
        b = as_form(b)
    except TypeError:
        return NotImplemented
    mesh = _join(a, b)
    if op in ('add', 'sub'):
        if a.shape != b.shape:
            raise ValueError('%s of shapes %r and %r' % (op, a.shape, b.shape))
        f = s_add if op == 'add' else s_sub
        return FormExpr(_map2(f, a.comps, b.comps, a.shape), a.shape,
                        max(a.deg, b.deg), mesh)
    if op == 'div':
        if b.shape:
            raise ValueError('division by a tensor of shape %r' % (b.shape,))
        return FormExpr(_map(lambda n: s_div(n, b.comps), a.comps, a.shape),
                        a.shape, a.deg + b.deg, mesh)
    # product: scalar scaling, matrix-vector or matrix-matrix
    deg = a.deg + b.deg
    if not a.shape:
        return FormExpr(_map(lambda n: s_mul(a.comps, n), b.comps, b.shape),
                        b.shape, deg, mesh)
    if not b.shape:
        return FormExpr(_map(lambda n: s_mul(n, b.comps), a.comps, a.shape),
                        a.shape, deg, mesh)
    if len(a.shape) == 2:
        return _contract(a, b, deg, mesh)
    raise ValueError('product of shapes %r and %r: use dot or inner'
                     % (a.shape, b.shape))


def _contract(a, b, deg, mesh):
    '''a . b over the last index of a and the first of b.'''
    def sdot(x, y):
        return s_add(s_mul(x[0], y[0]), s_mul(x[1], y[1]))

    if len(a.shape) == 1 and len(b.shape) == 1:
        return FormExpr(sdot(a.comps, b.comps), (), deg, mesh)
    if len(a.shape) == 2 and len(b.shape) == 1:
        return FormExpr([sdot(a.comps[i], b.comps) for i in range(2)], (2,),
                        deg, mesh)
    bt = [[b.comps[0][j], b.comps[1][j]] for j in range(2)] \
        if len(b.shape) == 2 else None
    if len(a.shape) == 1:
        return FormExpr([sdot(a.comps, bt[j]) for j in range(2)], (2,), deg,
                        mesh)
    return FormExpr([[sdot(a.comps[i], bt[j]) for j in range(2)]
                     for i in range(2)], (2, 2), deg, mesh)


def _power(a, p):
    try:
        a = as_form(a)
    except TypeError:
        return NotImplemented
    if a.shape:
        raise ValueError('power of a tensor of shape %r' % (a.shape,))
    if isinstance(p, numbers.Integral) and not isinstance(p, bool):
        n = int(p)
        # (UFL: n * deg for n >= 0, else deg + 2)
        return FormExpr(s_powi(a.comps, n), (), n * a.deg if n >= 0
                        else a.deg + 2, a.mesh)
    if isinstance(p, numbers.Real) and float(p).is_integer() \
            and abs(p) <= 64:
        # a float exponent: UFL's estimate, the exact multiplies
        return FormExpr(s_powi(a.comps, int(p)), (), a.deg + 2, a.mesh)
    try:
        e = as_form(p)
    except TypeError:
        return NotImplemented
    if e.shape:
        raise ValueError('exponent of shape %r' % (e.shape,))
    return FormExpr(('pow', a.comps, e.comps), (), a.deg + 2,
                    _join_mesh(a.mesh, e.mesh))


def _function(name, f):
    f = as_form(f)
    if f.shape:
        raise ValueError('%s of a tensor of shape %r' % (name, f.shape))
    return FormExpr((name, f.comps), (),
                    f.deg if name in ('abs', 'sign') else f.deg + 2, f.mesh)


def sqrt(f):
    return _function('sqrt', f)


def exp(f):
    return _function('exp', f)


def ln(f):
    return _function('ln', f)


def sin(f):
    return _function('sin', f)


def cos(f):
    return _function('cos', f)


def tanh(f):
    return _function('tanh', f)


def sign(f):
    '''-1, 0 or 1 (degree unchanged, derivative 0).'''
    return _function('sign', f)


def _clip(name, a, b):
    a, b = as_form(a), as_form(b)
    if a.shape or b.shape:
        raise ValueError('%s_value of tensors of shapes %r and %r'
                         % (name, a.shape, b.shape))
    return FormExpr((name, a.comps, b.comps), (), max(a.deg, b.deg),
                    _join(a, b))


def max_value(a, b):
    return _clip('max', a, b)


def min_value(a, b):
    return _clip('min', a, b)


class Condition(object):
    '''lt(a, b) ... ne(a, b) and their And / Or / Not: what conditional()
    branches on.  Its tree is worth 1.0 or 0.0 on the device, but a condition
    is not a scalar operand: arithmetic with it is a TypeError.'''
    REFUSAL = ('a condition (lt, le, gt, ge, eq, ne, And, Or, Not) is not a '
               'scalar operand: use it as the first argument of conditional()')

    def __init__(self, tree, mesh):
        self.tree = tree
        self.mesh = mesh

    def _refuse(self, *args, **kwargs):
        raise TypeError(Condition.REFUSAL)

    __add__ = __radd__ = __sub__ = __rsub__ = __mul__ = __rmul__ = _refuse
    __truediv__ = __rtruediv__ = __div__ = __rdiv__ = _refuse
    __pow__ = __rpow__ = __neg__ = __pos__ = __abs__ = __float__ = _refuse
    __getitem__ = _refuse

    def __bool__(self):
        raise TypeError('a condition has no truth value on the host: it is '
                        'evaluated at the quadrature points (conditional())')

    __nonzero__ = __bool__


def _compare(name, a, b):
    a, b = as_form(a), as_form(b)
    if a.shape or b.shape:
        raise ValueError('%s of tensors of shapes %r and %r: conditions '
                         'compare scalars' % (name, a.shape, b.shape))
    return Condition((name, a.comps, b.comps), _join(a, b))


def lt(a, b):
    return _compare('lt', a, b)


def le(a, b):
    return _compare('le', a, b)


def gt(a, b):
    return _compare('gt', a, b)


def ge(a, b):
    return _compare('ge', a, b)


def eq(a, b):
    return _compare('eq', a, b)


def ne(a, b):
    return _compare('ne', a, b)


def _condition(c):
    if not isinstance(c, Condition):
        raise TypeError('a condition is expected: lt, le, gt, ge, eq, ne of '
                        'two scalars or And, Or, Not of conditions (got %r)'
                        % (type(c),))
    return c


def And(a, b):
    '''Both: the product of the two 0-1 values.'''
    a, b = _condition(a), _condition(b)
    return Condition(('mul', a.tree, b.tree), _join_mesh(a.mesh, b.mesh))


def Or(a, b):
    '''Either: the larger of the two 0-1 values.'''
    a, b = _condition(a), _condition(b)
    return Condition(('max', a.tree, b.tree), _join_mesh(a.mesh, b.mesh))


def Not(a):
    a = _condition(a)
    return Condition(('sub', ONE, a.tree), a.mesh)


def conditional(cond, t, f):
    '''t where cond holds, f elsewhere; tensors of equal shape component by
    component.  Degree: the larger of the branches'.  Both branches are
    computed, the result is SELECTED: a value of the untaken branch (inf,
    NaN) never reaches it.'''
    cond = _condition(cond)
    t, f = as_form(t), as_form(f)
    if t.shape != f.shape:
        raise ValueError('conditional of shapes %r and %r'
                         % (t.shape, f.shape))
    mesh = _join_mesh(cond.mesh, _join(t, f))
    return FormExpr(_map2(lambda x, y: s_cond(cond.tree, x, y), t.comps,
                          f.comps, t.shape), t.shape, max(t.deg, f.deg), mesh)


def _cell_quantity(mesh, k):
    if not _is_mesh(mesh):
        raise TypeError('%s takes a mesh (got %r)'
                        % (('CellVolume', 'Circumradius', 'CellDiameter')[k],
                           type(mesh)))
    return FormExpr(('cell', mesh, k), (), 0, mesh)


def CellVolume(mesh):
    '''|T| of the cell (of the owning cell under ds and at points): a
    cell-wise constant, degree 0, derivatives zero.'''
    return _cell_quantity(mesh, 0)


def Circumradius(mesh):
    '''abc / (4 |T|) of the cell's edge lengths a, b, c.'''
    return _cell_quantity(mesh, 1)


def CellDiameter(mesh):
    '''The largest distance between two vertices of the cell.'''
    return _cell_quantity(mesh, 2)


def dot(a, b):
    a, b = as_form(a), as_form(b)
    mesh = _join(a, b)
    if not a.shape or not b.shape:
        if a.shape or b.shape:
            raise ValueError('dot of shapes %r and %r' % (a.shape, b.shape))
        return _binary('mul', a, b)
    return _contract(a, b, a.deg + b.deg, mesh)


def inner(a, b):
    a, b = as_form(a), as_form(b)
    if a.shape != b.shape:
        raise ValueError('inner of shapes %r and %r' % (a.shape, b.shape))
    mesh = _join(a, b)
    total = ZERO
    for x, y in zip(a.scalar_trees(), b.scalar_trees()):
        total = s_add(total, s_mul(x, y))
    return FormExpr(total, (), a.deg + b.deg, mesh)


def grad(f):
    f = as_form(f)
    if len(f.shape) == 2:
        raise ValueError('grad of a rank-2 tensor would be rank 3: at most '
                         'rank 2 is supported')
    comps = _map(lambda n: [s_diff(n, 0), s_diff(n, 1)], f.comps, f.shape)
    return FormExpr(comps, f.shape + (2,), max(f.deg - 1, 0), f.mesh)


def div(f):
    f = as_form(f)
    if not f.shape:
        raise ValueError('div of a scalar')
    if len(f.shape) == 1:
        c = s_add(s_diff(f.comps[0], 0), s_diff(f.comps[1], 1))
    else:
        c = [s_add(s_diff(f.comps[i][0], 0), s_diff(f.comps[i][1], 1))
             for i in range(2)]
    return FormExpr(c, f.shape[1:], max(f.deg - 1, 0), f.mesh)


def curl(f):
    '''2-D: of a vector v the scalar dv1/dx - dv0/dy, of a scalar s the
    vector (ds/dy, -ds/dx).'''
    f = as_form(f)
    deg = max(f.deg - 1, 0)
    if not f.shape:
        return FormExpr([s_diff(f.comps, 1), s_neg(s_diff(f.comps, 0))], (2,),
                        deg, f.mesh)
    if len(f.shape) != 1:
        raise ValueError('curl of a tensor of shape %r' % (f.shape,))
    return FormExpr(s_sub(s_diff(f.comps[1], 0), s_diff(f.comps[0], 1)), (),
                    deg, f.mesh)


def as_vector(items):
    items = list(items)
    if len(items) != 2:
        raise ValueError('as_vector: 2 components in 2-D, got %d' % len(items))
    if all(isinstance(i, (list, tuple)) for i in items):
        rows = [as_vector(i) for i in items]
        if any(r.shape != (2,) for r in rows):
            raise ValueError('as_vector: rows must be vectors of scalars')
        return FormExpr([r.comps for r in rows], (2, 2),
                        max(r.deg for r in rows),
                        _join_mesh(rows[0].mesh, rows[1].mesh))
    parts = [as_form(i) for i in items]
    if any(p.shape for p in parts):
        raise ValueError('as_vector of non-scalar components (shapes %r)'
                         % ([p.shape for p in parts],))
    return FormExpr([p.comps for p in parts], (2,), max(p.deg for p in parts),
                    _join_mesh(parts[0].mesh, parts[1].mesh))


def _matrix(A, what):
    A = as_form(A)
    if A.shape != (2, 2):
        raise ValueError('%s of a tensor of shape %r: a 2 x 2 tensor is '
                         'expected' % (what, A.shape))
    return A


def transpose(A):
    '''A^T of a rank-2 tensor (also A.T).'''
    A = _matrix(A, 'transpose')
    return FormExpr([[A.comps[j][i] for j in range(2)] for i in range(2)],
                    (2, 2), A.deg, A.mesh)


def sym(A):
    '''(A + A^T) / 2.'''
    A = _matrix(A, 'sym')
    half = ('num', 0.5)
    return FormExpr([[A.comps[i][j] if i == j else
                      s_mul(half, s_add(A.comps[i][j], A.comps[j][i]))
                      for j in range(2)] for i in range(2)], (2, 2), A.deg,
                    A.mesh)


def tr(A):
    '''The trace A[0, 0] + A[1, 1].'''
    A = _matrix(A, 'tr')
    return FormExpr(s_add(A.comps[0][0], A.comps[1][1]), (), A.deg, A.mesh)


def Identity(dim):
    '''The dim x dim unit tensor (dim = 2: the meshes are 2-D).'''
    if dim != 2:
        raise ValueError('Identity(%r): the mesh is 2-D' % (dim,))
    return FormExpr([[ONE, ZERO], [ZERO, ONE]], (2, 2), 0)


def outer(a, b):
    '''The rank-2 tensor a_i b_j of two vectors.'''
    a, b = as_form(a), as_form(b)
    if a.shape != (2,) or b.shape != (2,):
        raise ValueError('outer of shapes %r and %r: two vectors are expected'
                         % (a.shape, b.shape))
    return FormExpr([[s_mul(a.comps[i], b.comps[j]) for j in range(2)]
                     for i in range(2)], (2, 2), a.deg + b.deg, _join(a, b))


def SpatialCoordinate(mesh):
    return FormExpr([('x', 0), ('x', 1)], (2,), 1, mesh)


def FacetNormal(mesh):
    '''The outward unit normal of the domain: ds integrands only (constant on
    every facet of an affine mesh, degree 0).'''
    return FormExpr([('n', 0), ('n', 1)], (2,), 0, mesh)


def _argument(V, number):
    name = ('TestFunction', 'TrialFunction')[number]
    if not hasattr(V, 'layout') or not hasattr(V, 'dim'):
        if mixed_arguments.enabled:
            # (a 3-vector does not exist here: the pair, as TestFunctions)
            raise NotImplementedError(
                '%s on a mixed space: take the pair, %ss(W)' % (name, name))
        raise NotImplementedError(
            '%s on a mixed space: only scalar P1 / P2 spaces carry arguments'
            % name)
    vector = vector_arguments.enabled and V.dim == 2 and V.component is None
    if (V.dim != 1 or V.component is not None) and not vector:
        raise NotImplementedError(
            '%s on a vector space or a component view: only scalar P1 / P2 '
            'spaces carry arguments' % name)
    if V.degree not in (1, 2):
        raise ValueError('%s: spaces of degree 1 or 2 only' % name)
    if vector:
        return FormExpr([('arg', number, 0, V, c) for c in range(2)], (2,),
                        V.degree, V.mesh())
    return FormExpr(('arg', number, 0, V), (), V.degree, V.mesh())


class _Switch(object):
    '''An opt-in switch of the process: `switch(True)` takes effect at
    construction, `.previous` is the setting it replaced, and as a context
    manager it restores that on exit.  Every subclass owns its `enabled`.'''
    enabled = False

    def __init__(self, on=True):
        self.previous = type(self).enabled
        type(self).enabled = bool(on)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        type(self).enabled = self.previous
        return False


class vector_arguments(_Switch):
    '''The switch of test and trial functions on vector spaces (2x2-block
    forms: elasticity, grad-div, the vector Laplacian).  Off by default:
    TestFunction(W) on a VectorFunctionSpace stays the NotImplementedError it
    was.  `vector_arguments(True)` switches them on at once, for the process;
    `.previous` is the setting it replaced, and as a context manager it
    restores that on exit.  `vector_arguments.enabled` is the current
    setting.'''
    enabled = False


class vector_derivatives(_Switch):
    '''The switch of derivative() with respect to a Function of a P1 / P2
    VectorFunctionSpace and of solve(F == 0) there (block Newton).  Off by
    default: both stay the NotImplementedError they were.
    `vector_derivatives(True)` switches them on at once, for the process;
    `.previous` is the setting it replaced, and as a context manager it
    restores that on exit.  `vector_derivatives.enabled` is the current
    setting.  The derivative is a form of vector arguments, so
    vector_arguments(True) is needed as well.'''
    enabled = False


_VECTOR_ARGUMENTS_OFF = (
    'vector_derivatives(True) is on, but vector_arguments(True) is not: the '
    'derivative with respect to a Function of a vector space is a form of '
    'test and trial functions on that space, which vector_arguments switches '
    'on')


def TestFunction(V):
    '''The test function of the space V (argument number 0): a scalar, or
    with vector_arguments(True) the 2-vector of a vector space.'''
    return _argument(V, 0)


def TrialFunction(V):
    '''The trial function of the space V (argument number 1).'''
    return _argument(V, 1)


class mixed_arguments(_Switch):
    '''The switch of test and trial functions, and of Functions, on a
    Taylor-Hood space WP = FunctionSpace(mesh, VectorElement('Lagrange',
    triangle, kv) * FiniteElement('Lagrange', triangle, kp)), kv, kp in {1,
    2}: TestFunctions(WP), TrialFunctions(WP), Function(WP), split.  Off by
    default: each of them stays the error it was.  `mixed_arguments(True)`
    switches them on at once, for the process; `.previous` is the setting it
    replaced, and as a context manager it restores that on exit.  It implies
    no other switch: the forms need vector_arguments(True) as well, their ds
    parts facet_arguments(True), their dx(k) parts cell_subdomains(True).'''
    enabled = False


class mixed_gmres(_Switch):
    '''The switch of solve(a == L, w, bcs) for NON-symmetric forms on a
    Taylor-Hood space (Oseen, Picard steps of Navier-Stokes, a Stokes form
    written with +q*div(u)): flexible GMRES with a block-triangular
    preconditioner over the one-launch block product (fem/mixed.py: fgmres,
    BlockTriangularPreconditioner, MixedMatrix.apply_fused).  Off by default:
    such a solve stays the NotImplementedError it was.  `mixed_gmres(True)`
    switches it on at once, for the process; `.previous` is the setting it
    replaced, and as a context manager it restores that on exit.  It implies
    no other switch.'''
    enabled = False


class mixed_derivatives(_Switch):
    '''The switch of derivative() with respect to a Function w of a
    Taylor-Hood space and of solve(F == 0, w, bcs) there (mixed Newton:
    fem/mixed.py, MixedNewtonAssembler, newton_solve).  Off by default: both
    stay the NotImplementedError they were.  `mixed_derivatives(True)`
    switches them on at once, for the process; `.previous` is the setting it
    replaced, and as a context manager it restores that on exit.  It implies
    no other switch: the forms need mixed_arguments(True) and
    vector_arguments(True), the linear solves of Newton's method
    mixed_gmres(True), ds parts facet_arguments(True), dx(k) parts
    cell_subdomains(True).'''
    enabled = False


_MIXED_MISMATCH = (
    'an argument of a mixed space together with an argument of another space '
    'in one form: the test and the trial function of a mixed form both come '
    'from TestFunctions(W) / TrialFunctions(W) of ONE mixed space')


def is_mixed_space(V):
    '''Whether V is a mixed (velocity-pressure) space.'''
    return hasattr(V, 'spaces') and not hasattr(V, 'layout')


def _mixed_arguments(W, number):
    name = ('TestFunctions', 'TrialFunctions')[number]
    if not is_mixed_space(W):
        raise NotImplementedError(
            '%s takes a mixed (velocity-pressure) space and returns a pair; '
            'on a scalar or vector space use %s' % (name, name[:-1]))
    if not mixed_arguments.enabled:
        # (the error TestFunction(W) / TrialFunction(W) always was)
        return _argument(W, number)
    if not vector_arguments.enabled:
        raise NotImplementedError(
            '%s: mixed_arguments(True) is on, but vector_arguments(True) is '
            'not: the velocity part is a vector argument, which '
            'vector_arguments switches on' % name)
    Wv, P = W.taylor_hood()
    mesh = W.mesh()
    v = FormExpr([('arg', number, 0, W, c) for c in range(2)], (2,),
                 Wv.degree, mesh)
    q = FormExpr(('arg', number, 0, W, 2), (), P.degree, mesh)
    return v, q


def TestFunctions(W):
    '''(v, q) of the Taylor-Hood space W (mixed_arguments(True)): the vector
    test function of the velocity part, a FormExpr of shape (2,), and the
    scalar one of the pressure part.  The leaves are ('arg', 0, d, W, comp),
    comp 0, 1 (velocity) or 2 (pressure); every component has its own scalar
    layout: W.sub(0)'s for 0 and 1, W.sub(1)'s for 2.'''
    return _mixed_arguments(W, 0)


def TrialFunctions(W):
    '''(u, p) of the Taylor-Hood space W: the trial functions (number 1).'''
    return _mixed_arguments(W, 1)


def split(w):
    '''split(w) of a Function on a mixed space: w.split(), views of its
    storage as ordinary Functions (coefficients of forms like any other).'''
    if not isinstance(w, Function) or not is_mixed_space(w.function_space()):
        raise TypeError('split takes a Function of a mixed space: the pairs '
                        'of test and trial functions come from '
                        'TestFunctions(W) / TrialFunctions(W)')
    return w.split()


def _same_space(V, W):
    if is_mixed_space(V) != is_mixed_space(W):
        raise NotImplementedError(_MIXED_MISMATCH)
    return V is W or V.same_as(W)


def arguments(n, found=None):
    '''{number: space} of the argument leaves of a scalar tree.'''
    found = {} if found is None else found
    if n[0] == 'arg':
        V = found.setdefault(n[1], n[3])
        if V is not n[3] and not _same_space(V, n[3]):
            raise NotImplementedError(
                'two %s functions of different spaces in one form'
                % ('test', 'trial')[n[1]])
    elif n[0] in NONLEAF:
        for c in n[1:]:
            if isinstance(c, tuple):
                arguments(c, found)
    return found


_OP_NAMES = {'powi': '**', 'pow': '**', 'div': '/', 'mul': '*',
             'max': 'max_value', 'min': 'min_value', 'cond': 'conditional',
             'lt': 'a condition (lt)', 'le': 'a condition (le)',
             'gt': 'a condition (gt)', 'ge': 'a condition (ge)',
             'eq': 'a condition (eq)', 'ne': 'a condition (ne)'}


def extract_arguments(n):
    '''The integrand tree n, linear in its arguments, as a table
    {(b, a): c}: n = sum c D_a u D_b v with argument-free trees c; b (test)
    and a (trial) are 0 value, 1 d/dx, 2 d/dy, or None where that argument is
    absent.  Arguments of a vector space: the keys are ((b, r), (a, s)), n =
    sum c D_a u_s D_b v_r with r the test and s the trial component.  Entries
    whose coefficient folds to zero are dropped.  ValueError, naming the
    operation, where n is not linear in an argument.'''
    k = n[0]
    if k == 'arg':
        # (a component of a vector argument: (derivative, component))
        d = n[2] if len(n) == 4 else (n[2], n[4])
        return {((d, None) if n[1] == 0 else (None, d)): ONE}
    if not has_leaf(n, 'arg'):
        return {} if _is_num(n, 0.0) else {(None, None): n}
    if k in ('add', 'sub'):
        out = dict(extract_arguments(n[1]))
        for key, c in extract_arguments(n[2]).items():
            if key in out:
                out[key] = (s_add if k == 'add' else s_sub)(out[key], c)
            else:
                out[key] = c if k == 'add' else s_neg(c)
        return out
    if k == 'neg':
        return {key: s_neg(c) for key, c in extract_arguments(n[1]).items()}
    if k == 'mul':
        out = {}
        tb = extract_arguments(n[2])
        for (b1, a1), c1 in extract_arguments(n[1]).items():
            for (b2, a2), c2 in tb.items():
                if (b1 is not None and b2 is not None) or (
                        a1 is not None and a2 is not None):
                    raise ValueError(
                        'the form is not linear: the %s function appears twice '
                        'in a product (*)'
                        % ('test' if b1 is not None and b2 is not None
                           else 'trial'))
                key = (b1 if b2 is None else b2, a1 if a2 is None else a2)
                c = s_mul(c1, c2)
                out[key] = s_add(out[key], c) if key in out else c
        return {key: c for key, c in out.items() if not _is_num(c, 0.0)}
    if k == 'div':
        if has_leaf(n[2], 'arg'):
            raise ValueError('the form is not linear: division (/) by an '
                             'expression of a test or trial function')
        return {key: s_div(c, n[2])
                for key, c in extract_arguments(n[1]).items()}
    if k == 'cond':
        # the conditional distributes over the two branches' tables: zero
        # where a branch lacks the term
        if has_leaf(n[1], 'arg'):
            raise ValueError('the form is not linear: a test or trial '
                             'function in the condition of a conditional')
        tt, tf = extract_arguments(n[2]), extract_arguments(n[3])
        out = {}
        for key in list(tt) + [key for key in tf if key not in tt]:
            c = s_cond(n[1], tt.get(key, ZERO), tf.get(key, ZERO))
            if not _is_num(c, 0.0):
                out[key] = c
        return out
    raise ValueError('the form is not linear: a test or trial function under '
                     '%s' % _OP_NAMES.get(k, k))


def argument_table(integrand):
    '''(rank, table) of a scalar integrand: table[b][a] (rank 2) or table[b]
    (rank 1) of coefficient trees, None where the term is absent.  With
    arguments of a vector space (callers tell by the space's dim) one such
    table per block: table[r][s][b][a] or table[r][b], None for an absent
    block.  Arguments of a mixed space (TestFunctions): a MixedTable of 3 x 3
    (rank 2) or 3 (rank 1) blocks over the components 0, 1 (velocity), 2
    (pressure).'''
    tab = {key: c for key, c in extract_arguments(integrand).items()
           if not _is_num(c, 0.0)}
    kinds = set((b is not None, a is not None) for b, a in tab)
    if (False, True) in kinds:
        raise ValueError('a term of the form holds the trial function without '
                         'the test function')
    if len(kinds) > 1:
        raise ValueError(
            'the terms of the integrand differ in rank (the test function '
            'without the trial function, or neither, in a sum that elsewhere '
            'has both): write the parts as separate forms and split them '
            'with lhs() / rhs()')
    if not kinds or kinds == {(False, False)}:
        return 0, None
    if any(isinstance(b, tuple) for b, a in tab):
        mixed = any(is_mixed_space(V) for V in arguments(integrand).values())
        return _block_table(tab, 1 if kinds == {(True, False)} else 2,
                            3 if mixed else 2)
    if kinds == {(True, False)}:
        return 1, [tab.get((b, None)) for b in range(3)]
    return 2, [[tab.get((b, a)) for a in range(3)] for b in range(3)]


class BlockTable(list):
    '''The table of a form of vector arguments: table[r][s] (rank 2) or
    table[r] (rank 1).  A list; the type is what tells it from the table of
    a scalar form (is_symmetric_table).'''


class MixedTable(BlockTable):
    '''The table of a form of arguments on a Taylor-Hood space: 3 x 3 (rank
    2) or 3 (rank 1) blocks over the components 0, 1 (velocity) and 2
    (pressure).  velocity() is its [0:2][0:2] corner (rank 1: [0:2]): exactly
    the BlockTable of the same terms written on the velocity space alone.'''

    def velocity(self):
        corner = BlockTable(row[:2] if self.rank == 2 else row
                            for row in self[:2])
        corner.rank = self.rank
        return corner


def _block_table(tab, rank, nb=2):
    '''argument_table of vector arguments: table[r] (rank 1) or table[r][s]
    (rank 2), r the test and s the trial component, each the table of a
    scalar form or None where the block has no term.  nb = 3: the components
    of a mixed space, a MixedTable.'''
    if any(d is not None and not isinstance(d, tuple)
           for key in tab for d in key):
        raise NotImplementedError(
            'test and trial functions of different spaces (a vector and a '
            'scalar argument in one form)')
    kind = MixedTable if nb == 3 else BlockTable
    if rank == 1:
        blocks = [[tab.get(((b, r), None)) for b in range(3)]
                  for r in range(nb)]
        table = kind(t if any(c is not None for c in t) else None
                     for t in blocks)
    else:
        blocks = [[[[tab.get(((b, r), (a, s))) for a in range(3)]
                    for b in range(3)] for s in range(nb)] for r in range(nb)]
        table = kind(
            [t if any(c is not None for row in t for c in row) else None
             for t in row] for row in blocks)
    table.rank = rank
    return rank, table


def block_items(table, rank):
    '''[(p, block table)] of the present blocks of a vector form's table: p =
    2 r + s (rank 2) or r (rank 1).'''
    if rank == 1:
        return [(r, table[r]) for r in range(2) if table[r] is not None]
    return [(2 * r + s, table[r][s]) for r in range(2) for s in range(2)
            if table[r][s] is not None]


def is_symmetric_table(table):
    '''Structural symmetry of a rank-2 table: c[b][a] and c[a][b] are the same
    tree for every (a, b).  A BlockTable (2 x 2 blocks, vector arguments):
    c[r][s][b][a] and c[s][r][a][b] are.'''
    if isinstance(table, BlockTable):
        nb = len(table)         # (3: the MixedTable of a Taylor-Hood form)

        def entry(r, s, b, a):
            return None if table[r][s] is None else table[r][s][b][a]
        return all(entry(r, s, b, a) == entry(s, r, a, b)
                   for r in range(nb) for s in range(nb)
                   for b in range(3) for a in range(3))
    return all(table[b][a] == table[a][b] for b in range(3) for a in range(b))


def is_symmetric_form(form):
    '''Structural symmetry of a rank-2 form of mixed (or vector) arguments
    over ALL its parts: the reference writes its Stokes form as three
    integrals, of which -p*div(v)*dx alone is not symmetric but together with
    -q*div(u)*dx is.  The signed coefficient trees of entry (r, s, b, a),
    collected over the parts with their measure (type, subdomain, metadata),
    must be those of entry (s, r, a, b).'''
    entries = {}
    for sign, part in form.terms():
        _, table = part.argument_table()
        if not isinstance(table, BlockTable):
            table = [[table]]
        where = (part.integral_type, part.subdomain_id,
                 id(part.subdomain_data), sorted(part.metadata.items()))
        nb = len(table)
        for r in range(nb):
            for s in range(nb):
                if table[r][s] is None:
                    continue
                for b in range(3):
                    for a in range(3):
                        c = table[r][s][b][a]
                        if c is None:
                            continue
                        # (one spelling of the sign: a - f and a + (-1)*f)
                        sg = sign
                        while c[0] == 'neg':
                            sg, c = -sg, c[1]
                        if _is_num(c):
                            sg, c = 1.0, ('num', sg * c[1])
                        entries.setdefault((r, s, b, a), []).append(
                            (sg, c, where))
    for (r, s, b, a), found in entries.items():
        other = list(entries.get((s, r, a, b), []))
        if len(other) != len(found):
            return False
        for item in found:
            if item not in other:
                return False
            other.remove(item)
    return True


def has_normal(n):
    '''Whether a scalar tree reads the facet normal.'''
    if n[0] == 'n':
        return True
    return n[0] in NONLEAF and any(
        has_normal(c) for c in n[1:] if isinstance(c, tuple))


def has_leaf(n, kind):
    '''Whether a scalar tree holds a leaf of `kind` ('n', 'expr', ...).'''
    if n[0] == kind:
        return True
    return n[0] in NONLEAF and any(
        has_leaf(c, kind) for c in n[1:] if isinstance(c, tuple))


def point_program(expr):
    '''The register program of a rank <= 1 expression at points (Probes,
    u(x)): one output per component.  ValueError for rank 2, Expression
    leaves and FacetNormal.'''
    expr = as_form(expr)
    if len(expr.shape) > 1:
        raise ValueError('point evaluation of a tensor of shape %r: evaluate '
                         'its rows or components, e.g. f[0] or f[0, 1]'
                         % (expr.shape,))
    return compile_trees(expr.scalar_trees(), point=True)


def check_no_normal(expr, where):
    if any(has_normal(t) for t in expr.scalar_trees()):
        raise ValueError('FacetNormal is defined on exterior facets only: it '
                         'cannot be used in %s' % where)


# -- measure and forms -----------------------------------------------------------
def _quadrature_degree(params):
    if not params:
        return None
    q = params.get('quadrature_degree')
    return None if q is None else int(q)


def quadrature_scheme(*params):
    '''The 'quadrature_rule' of the first of the parameter dicts (form compiler
    parameters, then the measure's metadata) that names one: 'default' or
    'vertex'.'''
    for p in params:
        rule = (p or {}).get('quadrature_rule')
        if rule is not None:
            if rule not in ('default', 'vertex'):
                raise ValueError("quadrature_rule %r: 'default' or 'vertex'"
                                 % (rule,))
            return rule
    return 'default'


_INTEGRAL_TYPES = {'dx': 'cell', 'cell': 'cell', 'ds': 'exterior_facet',
                   'exterior_facet': 'exterior_facet'}
_INTERIOR_TYPES = ('dS', 'interior_facet')
_MEASURE_NAMES = {'cell': 'dx', 'exterior_facet': 'ds', 'interior_facet': 'dS'}


def _is_mesh(obj):
    return hasattr(obj, 'num_cells') and hasattr(obj, 'bfacets')


class interior_facets(_Switch):
    '''The switch of interior-facet integrals: dS, Measure('dS'), jump, avg,
    FacetArea and the restrictions f('+') / f('-').  Off by default: each of
    them stays the NotImplementedError it was.  `interior_facets(True)`
    switches them on at once, for the process; `.previous` is the setting it
    replaced, and as a context manager it restores that on exit.
    `interior_facets.enabled` is the current setting.'''
    enabled = False


_INTERIOR_FACETS_OFF = (
    'dS: interior-facet integrals (dS, jump, avg, FacetArea and the '
    "restrictions ('+') / ('-')) are off by default (dx and ds are "
    'supported); interior_facets(True) switches them on')


def _need_interior_facets():
    if not interior_facets.enabled:
        raise NotImplementedError(_INTERIOR_FACETS_OFF)


# -- restrictions, jump, avg ---------------------------------------------------
# The '+' cell of an interior facet is the one with the SMALLER cell index,
# the '-' cell the other (Mesh.interior_facets).  UFL's apply_restrictions
# rules: values of P1 / P2 Functions, SpatialCoordinate, Constants, numbers
# and FacetArea are continuous and may stand unrestricted under dS (they are
# evaluated on '+'); gradients of fields, FacetNormal, CellVolume,
# Circumradius and CellDiameter must be restricted.
_SIDES = {'+': 0, '-': 1}
_LEAF_NAMES = {'n': 'FacetNormal', 'expr': 'an Expression',
               'arg': 'a test or trial function'}


def _leaf_name(leaf):
    '''What the user wrote, for a message.'''
    if leaf[0] == 'field':
        name = getattr(leaf[1], 'name', None)
        name = name() if callable(name) else name
        what = 'a Function' if not name else 'the Function %r' % (name,)
        return what if leaf[3] == 0 else 'the gradient (grad, div, curl, ' \
            '.dx) of ' + what
    if leaf[0] == 'cell':
        return ('CellVolume', 'Circumradius', 'CellDiameter')[leaf[2]]
    return _LEAF_NAMES.get(leaf[0], leaf[0])


def _restrict(n, s):
    k = n[0]
    if k == 'side':
        raise ValueError('a restriction of a restricted expression: %s is '
                         "already restricted to ('%s')"
                         % (_leaf_name(n[1]), '+-'[n[2]]))
    if k in NONLEAF:
        return (k,) + tuple(_restrict(c, s) if isinstance(c, tuple) else c
                            for c in n[1:])
    if k in ('num', 'const', 'x', 'farea'):
        return n            # (the same on both sides)
    return ('side', n, s)


def restricted(f, side):
    '''f('+') / f('-') of a scalar, vector or tensor: every leaf that lives
    on a cell (field values and gradients, FacetNormal, cell geometry) is
    restricted to that side of the interior facet; numbers, Constants,
    SpatialCoordinate and FacetArea are the same on both.'''
    _need_interior_facets()
    if side not in _SIDES:
        raise ValueError("a restriction is ('+') or ('-'), got %r" % (side,))
    f = as_form(f)
    s = _SIDES[side]
    return FormExpr(_map(lambda n: _restrict(n, s), f.comps, f.shape),
                    f.shape, f.deg, f.mesh)


def jump(f, n=None):
    """jump(f) = f('+') - f('-'); jump(f, n) = f('+')*n('+') + f('-')*n('-')
    for a scalar f (a vector), dot(f('+'), n('+')) + dot(f('-'), n('-')) for a
    vector f (a scalar)."""
    _need_interior_facets()
    f = as_form(f)
    if n is None:
        return restricted(f, '+') - restricted(f, '-')
    n = as_form(n)
    if n.shape != (2,):
        raise ValueError('jump(f, n): n is the FacetNormal')
    if not f.shape:
        return restricted(f, '+') * restricted(n, '+') \
            + restricted(f, '-') * restricted(n, '-')
    if f.shape != (2,):
        raise ValueError('jump(f, n) of a tensor of shape %r: f is a scalar '
                         'or a vector' % (f.shape,))
    return dot(restricted(f, '+'), restricted(n, '+')) \
        + dot(restricted(f, '-'), restricted(n, '-'))


def avg(f):
    """(f('+') + f('-')) / 2."""
    _need_interior_facets()
    f = as_form(f)
    return (restricted(f, '+') + restricted(f, '-')) / 2


def FacetArea(mesh):
    '''The length of the facet: a scalar of degree 0, dS integrands only.'''
    _need_interior_facets()
    if not _is_mesh(mesh):
        raise TypeError('FacetArea takes a mesh (got %r)' % (type(mesh),))
    return FormExpr(('farea', mesh), (), 0, mesh)


def side_leaves(n, found=None):
    '''[(leaf, side)] of a scalar tree: every leaf, with the side (0 | 1) it
    is restricted to or None.'''
    found = [] if found is None else found
    if n[0] == 'side':
        found.append((n[1], n[2]))
    elif n[0] in NONLEAF:
        for c in n[1:]:
            if isinstance(c, tuple):
                side_leaves(c, found)
    else:
        found.append((n, None))
    return found


def _check_no_sides(tree, where):
    '''dx, ds, points, projections: no restriction, no FacetArea.'''
    for leaf, side in side_leaves(tree):
        if side is not None:
            raise ValueError(
                "a restriction ('+') / ('-') is defined on interior facets "
                'only: %s is restricted in %s' % (_leaf_name(leaf), where))
        if leaf[0] == 'farea':
            raise NotImplementedError(
                'FacetArea in %s: it is provided on interior facets (dS) only'
                % where)


def _interior_integrand(n):
    '''The tree of a dS integrand with the continuous operands that stand
    unrestricted evaluated on '+'; ValueError, naming the operand, for one
    that must be restricted.'''
    k = n[0]
    if k == 'side':
        leaf = n[1]
    elif k in NONLEAF:
        return (k,) + tuple(_interior_integrand(c) if isinstance(c, tuple)
                            else c for c in n[1:])
    else:
        leaf = n
    if leaf[0] == 'arg':
        raise NotImplementedError(
            'test and trial functions under dS: restricted arguments need '
            'twice the coefficient slots and, for rank 2, a sparsity pattern '
            "wider than the space's (DG and interior-penalty matrices are "
            'out of scope)')
    if leaf[0] == 'expr':
        raise NotImplementedError(
            'Expression operands and the SUPG tau under dS: their tables are '
            "indexed by the rule's row of ONE cell; interpolate the "
            'Expression into a Function')
    if k == 'side' or leaf[0] in ('num', 'const', 'x', 'farea'):
        return n
    if leaf[0] == 'field' and leaf[3] == 0:
        return ('side', leaf, 0)
    raise ValueError(
        "%s is discontinuous across an interior facet: restrict it, ('+') or "
        "('-'), or use jump / avg, in a dS integrand" % _leaf_name(leaf))


class facet_arguments(_Switch):
    '''The switch of test and trial functions under ds (Neumann, Robin and
    Nitsche terms).  Off by default: `v*ds` and derivative() of a ds part stay
    the NotImplementedError they were.  `facet_arguments(True)` switches them
    on at once, for the process; `.previous` is the setting it replaced, and
    as a context manager it restores that on exit.  `facet_arguments.enabled`
    is the current setting.'''
    enabled = False


_FACET_ARGUMENTS_OFF = (
    'test and trial functions under ds (Neumann and Robin terms): '
    'the facet gather needs a contribution map that is built only after '
    'facet_arguments(True); they are off by default')


class cell_subdomains(_Switch):
    '''The switch of cell subdomains: cell MeshFunctions (dim 2, CellFunction),
    SubDomain.mark on them, and `dx(k)` / `dx(subdomain_data=markers)` /
    Measure('dx', domain=mesh, subdomain_data=markers)(k) for forms of every
    rank.  Off by default: each of them stays the NotImplementedError it was.
    `cell_subdomains(True)` switches them on at once, for the process;
    `.previous` is the setting it replaced, and as a context manager it
    restores that on exit.  `cell_subdomains.enabled` is the current
    setting.'''
    enabled = False


def _check_markers(integral_type, subdomain_id, markers):
    '''ValueError for markers of the wrong kind (a facet MeshFunction under
    dx, a cell one under ds / dS) and for a subdomain id that is not one
    integer.'''
    name = _MEASURE_NAMES[integral_type]
    if markers is not None:
        dim = getattr(markers, 'dim', None)
        want = 2 if integral_type == 'cell' else 1
        if dim != want and (want == 2 or dim == 2):
            raise ValueError(
                '%s takes a %s MeshFunction (dim %d) as subdomain_data: got '
                '%s' % (name, 'cell' if want == 2 else 'facet', want,
                        'a %s MeshFunction (dim %d)'
                        % ('cell' if dim == 2 else 'facet', dim)
                        if dim in (1, 2) else repr(type(markers))))
    if integral_type == 'cell' and subdomain_id != 'everywhere' and (
            isinstance(subdomain_id, bool)
            or not isinstance(subdomain_id, numbers.Integral)):
        raise ValueError('dx(%r): a cell subdomain id is one integer (tuples '
                         'of ids are not provided)' % (subdomain_id,))


class Measure(object):
    '''`dx` over the cells, `ds` over the exterior facets (UFL's
    Measure(integral_type, domain, subdomain_id, metadata, subdomain_data)).
    Calls: `dx(mesh)`, `dx(domain=mesh)`, `dx(metadata={...})`, `dx(degree=q)`;
    `ds` also takes a subdomain id, `ds(1)` / `ds(subdomain_id=1)`, which
    selects the facets its subdomain_data (a facet MeshFunction) marks 1.
    With cell_subdomains(True) `dx` takes one too: `dx(1)` selects the cells
    its subdomain_data (a cell MeshFunction) marks 1.'''

    def __init__(self, integral_type='dx', domain=None,
                 subdomain_id='everywhere', metadata=None, subdomain_data=None):
        if integral_type in _INTERIOR_TYPES and interior_facets.enabled:
            self.integral_type = 'interior_facet'
        elif integral_type not in _INTEGRAL_TYPES:
            raise NotImplementedError(
                'integral type %r: only dx (cells) and ds (exterior facets) '
                'are supported; dS (interior facets) after '
                'interior_facets(True)' % (integral_type,))
        else:
            self.integral_type = _INTEGRAL_TYPES[integral_type]
        self.mesh = domain
        self.subdomain_id = subdomain_id
        self.metadata = dict(metadata or {})
        self.subdomain_data = subdomain_data
        if self.integral_type == 'cell' and (
                subdomain_id != 'everywhere' or subdomain_data is not None) \
                and not cell_subdomains.enabled:
            raise NotImplementedError('cell subdomains: dx integrates over '
                                      'the whole mesh')
        _check_markers(self.integral_type, subdomain_id, subdomain_data)

    def __call__(self, subdomain_id=None, metadata=None, domain=None,
                 subdomain_data=None, degree=None):
        if _is_mesh(subdomain_id):          # ds(mesh), dx(mesh)
            subdomain_id, domain = None, subdomain_id
        md = dict(self.metadata)
        md.update(metadata or {})
        if degree is not None:
            md['quadrature_degree'] = degree
        return Measure(
            _MEASURE_NAMES[self.integral_type],
            domain if domain is not None else self.mesh,
            self.subdomain_id if subdomain_id is None else subdomain_id, md,
            self.subdomain_data if subdomain_data is None else subdomain_data)

    def __rmul__(self, other):
        f = as_form(other)
        if f.shape:
            raise ValueError('only scalar integrands can be integrated: the '
                             'integrand has shape %r' % (f.shape,))
        if self.integral_type == 'interior_facet':
            tree = _interior_integrand(f.comps)
            mesh = _join_mesh(f.mesh, self.mesh)
            if self.subdomain_data is not None:
                mesh = _join_mesh(mesh, self.subdomain_data.mesh)
            return Form(FormExpr(tree, (), f.deg, f.mesh), mesh,
                        self.metadata, 'interior_facet', self.subdomain_id,
                        self.subdomain_data)
        _check_no_sides(f.comps, 'a %s integral'
                        % _MEASURE_NAMES[self.integral_type])
        if self.integral_type == 'cell':
            check_no_normal(f, 'a dx integral')
            mesh = _join_mesh(f.mesh, self.mesh)
            if self.subdomain_data is not None:
                if mesh is not None and self.subdomain_data.mesh is not mesh:
                    raise ValueError('the cell markers of dx belong to '
                                     'another mesh than the integrand')
                mesh = self.subdomain_data.mesh
            return Form(f, mesh, self.metadata, 'cell', self.subdomain_id,
                        self.subdomain_data)
        if has_leaf(f.comps, 'arg') and not facet_arguments.enabled:
            raise NotImplementedError(_FACET_ARGUMENTS_OFF)
        if has_leaf(f.comps, 'arg') and quadrature_scheme(
                self.metadata) == 'vertex':
            raise ValueError(
                "quadrature_rule 'vertex' on a ds part with test or trial "
                "functions: the vertex rule is a rule of cells")
        mesh = _join_mesh(f.mesh, self.mesh)
        if self.subdomain_data is not None:
            mesh = _join_mesh(mesh, self.subdomain_data.mesh)
        return Form(f, mesh, self.metadata, 'exterior_facet',
                    self.subdomain_id, self.subdomain_data)


dx = Measure('dx')
ds = Measure('ds')


class _InteriorFacets(object):
    """dS: the measure of the interior facets, Measure('dS'), once
    interior_facets(True) has switched it on; the NotImplementedError it
    always was until then."""

    def _measure(self):
        _need_interior_facets()
        return Measure('dS')

    def __call__(self, *args, **kwargs):
        return self._measure()(*args, **kwargs)

    def __rmul__(self, other):
        return self._measure().__rmul__(other)


dS = _InteriorFacets()


class Form(object):
    '''A form: a scalar integrand over the cells of a mesh (integral_type
    'cell') or over its exterior facets ('exterior_facet': all of them for
    subdomain_id 'everywhere', else those whose subdomain_data marker equals
    subdomain_id).  `rank` counts its arguments: 0 a functional, 1 linear in
    a test function, 2 bilinear in a trial and a test function.  Forms add
    and subtract into a FormSum; `a == L` is an Equation when a side has
    arguments.'''

    def __init__(self, integrand, mesh, metadata, integral_type='cell',
                 subdomain_id='everywhere', subdomain_data=None):
        self.integrand = integrand
        self.mesh = mesh
        self.metadata = metadata
        self.integral_type = integral_type
        self.subdomain_id = subdomain_id
        self.subdomain_data = subdomain_data

    def degree(self):
        q = _quadrature_degree(self.metadata)
        return self.integrand.deg if q is None else q

    def terms(self):
        return [(1.0, self)]

    def arguments(self):
        '''{number: space} of the test (0) and trial (1) functions.'''
        if getattr(self, '_arguments', None) is None:
            found = arguments(self.integrand.comps)
            if 0 in found and 1 in found \
                    and not _same_space(found[0], found[1]):
                raise NotImplementedError(
                    'test and trial functions of different spaces or meshes')
            self._arguments = found
        return self._arguments

    def argument_table(self):
        '''(rank, coefficient table) of the integrand: argument_table().'''
        if getattr(self, '_table', None) is None:
            self.arguments()
            self._table = argument_table(self.integrand.comps)
        return self._table

    @property
    def rank(self):
        if not has_leaf(self.integrand.comps, 'arg'):
            return 0
        return self.argument_table()[0]

    def function_space(self):
        '''The space of the test function (None for a functional).'''
        return self.arguments().get(0)

    def __eq__(self, other):
        if isinstance(other, Form) and (_sum_rank(self) or _sum_rank(other)):
            return Equation(self, other)
        if isinstance(other, numbers.Real) and not isinstance(other, bool):
            if other != 0:
                raise ValueError('F == %r: a form equals another form (a == L) '
                                 'or 0 (the nonlinear F == 0)' % (other,))
            return Equation(self, 0)
        return NotImplemented

    __hash__ = object.__hash__

    def __add__(self, other):
        return FormSum.of(self, other, 1.0)

    def __radd__(self, other):
        if isinstance(other, numbers.Real) and other == 0:     # sum([...])
            return FormSum(self.terms())
        return NotImplemented

    def __sub__(self, other):
        return FormSum.of(self, other, -1.0)

    def __neg__(self):
        return FormSum([(-s, f) for s, f in self.terms()])


class FormSum(Form):
    '''A signed sum of forms; assemble() adds the parts in the order they
    were written.  The parts of an assembled sum have one rank; lhs() / rhs()
    split a sum that mixes ranks 1 and 2.'''

    def __init__(self, terms):
        self._terms = list(terms)

    @staticmethod
    def of(a, b, sign):
        if not isinstance(b, Form):
            return NotImplemented
        return FormSum(a.terms() + [(sign * s, f) for s, f in b.terms()])

    def terms(self):
        return list(self._terms)

    def degree(self):
        raise TypeError('a sum of forms has one degree per part')

    def arguments(self):
        found = {}
        for _, f in self._terms:
            for number, V in f.arguments().items():
                W = found.setdefault(number, V)
                if not _same_space(W, V):
                    raise NotImplementedError(
                        'test and trial functions of different spaces or '
                        'meshes')
        return found

    @property
    def rank(self):
        ranks = set(f.rank for _, f in self._terms)
        if len(ranks) > 1:
            raise ValueError('the parts of the sum have ranks %s: split it '
                             'with lhs() and rhs()' % sorted(ranks))
        return ranks.pop() if ranks else 0

    def argument_table(self):
        raise TypeError('a sum of forms has one table per part')


def _sum_rank(form):
    '''The highest rank among the parts of a form or sum.'''
    return max([f.rank for _, f in form.terms()] or [0])


class Equation(object):
    '''`a == L`, or `F == 0` (rhs the number 0): what solve() takes.'''

    def __init__(self, lhs, rhs):
        self.lhs = lhs
        self.rhs = rhs

    def __bool__(self):
        # (as UFL: `if a == L` asks whether the two are the same object)
        return self.lhs is self.rhs

    __nonzero__ = __bool__


def _parts_of_rank(form, rank, sign):
    if not isinstance(form, Form):
        raise TypeError('lhs / rhs / system take a form (got %r)'
                        % (type(form),))
    parts = []
    for s, f in form.terms():
        if not has_leaf(f.integrand.comps, 'arg'):
            raise ValueError('lhs / rhs / system: a part of the sum has no '
                             'test function')
        f.arguments()
        tab = {key: c for key, c in
               extract_arguments(f.integrand.comps).items()
               if not _is_num(c, 0.0)}
        ranks = set((b is not None) + (a is not None) for b, a in tab)
        if len(ranks) <= 1 or 0 in ranks \
                or any(b is None for b, a in tab):
            # one rank (or an integrand argument_table refuses, with its
            # message): the part as it was written
            if f.rank == 0:
                raise ValueError('lhs / rhs / system: a part of the sum has '
                                 'no test function')
            if f.rank == rank:
                parts.append((sign * s, f))
            continue
        # an integrand of both ranks, as the reference's SUPG term (R2 holds
        # the trial function and the source): split by linearity, as UFL does.
        # The terms of the wanted rank, c D_a u D_b v, at the degree of the
        # integrand they came from
        found = f.arguments()
        tree = ZERO
        for (b, a), c in tab.items():
            if (a is not None) + 1 != rank:
                continue
            term = s_mul(c, _arg_leaf(0, b, found[0]))
            if a is not None:
                term = s_mul(term, _arg_leaf(1, a, found[1]))
            tree = s_add(tree, term)
        if _is_num(tree, 0.0):
            continue
        split = Form(FormExpr(tree, (), f.integrand.deg, f.integrand.mesh),
                     f.mesh, f.metadata, f.integral_type, f.subdomain_id,
                     f.subdomain_data)
        parts.append((sign * s, split))
    return FormSum(parts)


def _arg_leaf(number, d, V):
    '''The argument leaf of a key of extract_arguments: d, or (d, comp).'''
    if isinstance(d, tuple):
        return ('arg', number, d[0], V, d[1])
    return ('arg', number, d, V)


def lhs(F):
    '''The bilinear parts of a signed sum of forms F (as UFL's lhs).'''
    return _parts_of_rank(F, 2, 1.0)


def rhs(F):
    '''The linear parts of F, NEGATED (as UFL's rhs: F = a - L = 0).'''
    return _parts_of_rank(F, 1, -1.0)


def system(F):
    return lhs(F), rhs(F)


def derivative(F, u, du=None):
    '''The Gateaux derivative of the form (or signed sum) F of rank 0 or 1
    with respect to the scalar P1 / P2 Function u (with
    vector_derivatives(True): or one of a vector space), part by part: a form of
    rank + 1 whose new argument has the number of arguments F already has (0:
    the test, 1: the trial function of u's space).  du: that argument, given
    explicitly.  See the module docstring for the rules and the refusals.
    With mixed_derivatives(True) u may be a Function of a Taylor-Hood space:
    _mixed_derivative.'''
    if not isinstance(F, Form):
        raise TypeError('derivative takes a form (got %r)' % (type(F),))
    if _sum_rank(F) >= 2:
        raise NotImplementedError(
            'derivative of a bilinear form would be a rank-3 form')
    if not isinstance(u, Function):
        raise TypeError('derivative with respect to a Function (got %r)'
                        % (type(u),))
    V = u.function_space()
    if is_mixed_space(V) and mixed_derivatives.enabled:
        return _mixed_derivative(F, u, du)
    plain = hasattr(V, 'layout') and hasattr(V, 'dim') \
        and V.component is None
    vector = plain and V.dim == 2 and vector_derivatives.enabled
    if not (plain and V.dim == 1) and not vector:
        raise NotImplementedError(
            'derivative with respect to a Function of a vector, component or '
            'mixed space: only scalar P1 / P2 spaces carry arguments')
    if vector and not vector_arguments.enabled:
        raise NotImplementedError(_VECTOR_ARGUMENTS_OFF)
    if V.degree not in (1, 2):
        raise ValueError('derivative: spaces of degree 1 or 2 only')
    found = F.arguments()
    k = len(found)
    if sorted(found) != list(range(k)):
        raise ValueError('derivative: the form holds a trial function without '
                         'a test function')
    for W in found.values():
        if not W.same_as(V):
            raise ValueError(
                'derivative: u and the arguments of the form live on '
                'different spaces or meshes')
    if du is not None:
        t = du.comps if isinstance(du, FormExpr) else None
        if vector:
            # (the 2-vector of leaves TestFunction(W) / TrialFunction(W) is)
            ok = du.shape == (2,) and all(
                c[:3] == ('arg', k, 0) and len(c) == 5 and c[3].same_as(V)
                and c[4] == i for i, c in enumerate(t)) \
                if t is not None else False
        else:
            ok = isinstance(t, tuple) and t[0] == 'arg' and t[1] == k \
                and t[2] == 0 and len(t) == 4 and t[3].same_as(V)
        if not ok:
            raise ValueError(
                'derivative: du must be the %s(V) of the space of u'
                % ('TestFunction', 'TrialFunction')[k])
    return _derived_parts(F, u, k, V)


def _mixed_derivative(F, w, du):
    '''derivative(F, w, du) for w a Function of a Taylor-Hood space WP
    (mixed_derivatives(True)): the fields of F that are views of w (w.split(),
    w.sub(i), split(w)) become the leaves of TrialFunctions(WP) -- or of
    TestFunctions(WP) for a rank-0 F --, so the result is a mixed form like a
    hand-written one.  A deep copy, or a view of another Function, is a
    coefficient and differentiates to zero.'''
    WP = w.function_space()
    if not getattr(w, '_mixed', False):
        raise ValueError('derivative: w was made before mixed_arguments(True) '
                         'and is no Function of the Taylor-Hood space')
    found = F.arguments()
    k = len(found)
    if sorted(found) != list(range(k)):
        raise ValueError('derivative: the form holds a trial function without '
                         'a test function')
    for W in found.values():
        if not (is_mixed_space(W) and W.same_as(WP)):
            raise ValueError(
                'derivative: w and the arguments of the form live on '
                'different spaces or meshes')
    if du is not None:
        name = ('TestFunctions', 'TrialFunctions')[k]
        ok = isinstance(du, (tuple, list)) and len(du) == 2 \
            and all(isinstance(e, FormExpr) for e in du)
        if ok:
            leaves = list(du[0].comps) if du[0].shape == (2,) else [None]
            leaves.append(du[1].comps if du[1].shape == () else None)
            ok = len(leaves) == 3 and all(
                isinstance(c, tuple) and len(c) == 5
                and c[:3] == ('arg', k, 0) and is_mixed_space(c[3])
                and c[3].same_as(WP) and c[4] == i
                for i, c in enumerate(leaves))
        if not ok:
            raise ValueError(
                'derivative: du must be the pair %s(W) of the space of w'
                % name)
    return _derived_parts(F, w, k, WP)


def _derived_parts(F, u, k, V):
    '''The parts of derivative(F, u): s_gateaux of every part of F in the
    direction of argument number k of V, with the degree, measure and
    subdomain of the part it came from.'''
    parts = []
    for sign, part in F.terms():
        if part.integral_type == 'interior_facet':
            raise NotImplementedError(
                'derivative of a dS part: the result would hold test or '
                'trial functions under dS')
        tree = s_gateaux(part.integrand.comps, u, k, V)
        if _is_num(tree, 0.0):
            continue
        if part.integral_type != 'cell' and not facet_arguments.enabled:
            raise NotImplementedError('derivative of a ds part: '
                                      + _FACET_ARGUMENTS_OFF)
        mesh = _join_mesh(_join_mesh(part.integrand.mesh, part.mesh),
                          V.mesh())
        # (the degree of the part it came from: see the module docstring)
        derived = Form(FormExpr(tree, (), part.integrand.deg, mesh), mesh,
                       part.metadata, part.integral_type, part.subdomain_id,
                       part.subdomain_data)
        derived.derived_from = part
        parts.append((sign, derived))
    if not parts:
        raise ValueError('derivative: the form does not depend on u')
    if len(parts) == 1 and parts[0][0] == 1.0 and not isinstance(F, FormSum):
        return parts[0][1]
    return FormSum(parts)


def action(*args, **kwargs):
    raise NotImplementedError('action(): assemble the form and multiply, '
                              'A * u, or write u in place of the trial '
                              'function')


def adjoint(*args, **kwargs):
    raise NotImplementedError('adjoint(): swap the test and trial functions '
                              'in the form by hand')


def check_degree(q):
    if not 0 <= q <= MAX_QUADRATURE_DEGREE:
        raise ValueError('quadrature degree %d: at most %d is supported'
                         % (q, MAX_QUADRATURE_DEGREE))
    return q


def projection_degree(expr, test_degree, form_compiler_parameters=None):
    q = _quadrature_degree(form_compiler_parameters)
    return check_degree(expr.deg + test_degree if q is None else q)


# -- register programs -----------------------------------------------------------
class ProgramLimit(ValueError):
    '''The trees exceed a limit of flow_form (instructions, registers,
    constants, field or Expression slots): what the callers with a fallback
    (compile_trees, argument_programs, the Newton assembler) catch.  A
    ValueError, as it always was.'''


class Program(object):
    '''Instructions (op, dst, a, b) over REGISTERS registers for a list of
    scalar trees (output k = tree k), and the operands they load: constants
    (('num', v) or (Constant, i)), field components (Function, i) and
    Expression components (Expression, i), in slot order.'''

    def __init__(self, trees, facet=False, point=False, slots=None,
                 nout=None, shared=(), interior=False):
        '''interior: the program runs on interior facets (dS), where a lane
        holds two cells: restricted leaves and FacetArea exist (ValueError
        otherwise), Expression leaves do not; every (Function, component,
        side) takes a field slot of its own, `field_sides` is the side of
        each.  facet: the program runs on exterior facets, where the normal
        exists (ValueError if a tree reads it otherwise).  point: it runs at
        located points (Probes, u(x)), where neither the normal nor
        Expression leaves exist (their lattices are tabulated at the rule's
        points only).  slots: the output slot of every tree out of nout
        (default: tree k -> output k of len(trees)); the coefficient tables
        of forms of arguments use it (argument_program).  shared: (register,
        tree) pairs computed first, in that order, into registers the output
        trees then read through ('reg', r) leaves (newton_program).'''
        trees = list(trees)
        shared = list(shared)
        if point and any(has_leaf(t, 'n') for t in trees):
            raise ValueError('FacetNormal is defined on exterior facets only: '
                             'it cannot be evaluated at points')
        if point and any(has_leaf(t, 'expr') for t in trees):
            raise ValueError('Expression leaves cannot be evaluated at points: '
                             'interpolate the Expression into a Function')
        if not interior:
            for t in trees + [t for _, t in shared]:
                _check_no_sides(t, 'a program of cells, exterior facets or '
                                'points')
        elif any(has_leaf(t, 'expr') for t in trees):
            raise ValueError('Expression leaves cannot be evaluated on '
                             'interior facets')
        facet = facet or interior
        if not facet and any(has_normal(t) for t in trees):
            raise ValueError('FacetNormal is defined on exterior facets only: '
                             'integrate over ds')
        if any(has_leaf(t, 'arg') for t in trees):
            raise ValueError('test and trial functions are not evaluated: only '
                             'their coefficients compile (argument_table)')
        if slots is None:
            slots = list(range(len(trees)))
        self.code = []
        self.consts = []
        self.fields = []
        # (interior: 0 '+' | 1 '-' per field slot; else None)
        self.field_sides = [] if interior else None
        self.exprs = []
        self.nregs = 0
        for r, t in shared:
            self._gen(t, 0)
            self._emit('mov', r, 0)
        for k, t in zip(slots, trees):
            self._gen(t, 0)
            self._emit('out', 0, 0, k)
        if len(self.code) > MAX_PROGRAM:
            raise ProgramLimit('the integrand compiles to %d instructions: the '
                             'limit is %d' % (len(self.code), MAX_PROGRAM))
        self.slots = list(slots)
        self.nout = len(trees) if nout is None else nout

    def signature(self):
        return (tuple(self.code),
                tuple(f.function_space().degree for f, _ in self.fields),
                tuple(int(e.degree) for e, _ in self.exprs))

    def _slot(self, table, key, limit, what):
        for i, k in enumerate(table):
            if k[0] is key[0] and k[1] == key[1]:
                return i
        if len(table) == limit:
            raise ProgramLimit('the integrand needs more than %d %s: the limit '
                             'is %d' % (limit, what, limit))
        table.append(key)
        return len(table) - 1

    def _emit(self, op, dst, a=0, b=0):
        if op != 'out':
            if dst >= REGISTERS:
                raise ProgramLimit('the integrand needs more than %d registers: '
                                 'the limit is %d' % (REGISTERS, REGISTERS))
            self.nregs = max(self.nregs, dst + 1)
        self.code.append((OPS[op], dst, a, b))

    def _const(self, key):
        for i, k in enumerate(self.consts):
            if (k[0] == 'num' and key[0] == 'num' and k[1] == key[1]) or (
                    k[0] is key[0] and k[1] == key[1]):
                return i
        if len(self.consts) == MAX_CONSTANTS:
            raise ProgramLimit('the integrand needs more than %d constants: the '
                             'limit is %d' % (MAX_CONSTANTS, MAX_CONSTANTS))
        self.consts.append(key)
        return len(self.consts) - 1

    @staticmethod
    def need(n):
        '''Registers the tree needs (Sethi-Ullman).'''
        k = n[0]
        if k in ('num', 'const', 'x', 'field', 'expr', 'n', 'reg', 'cell',
                 'side', 'farea'):
            return 1
        if k in UNARY + UNARY_EXT:
            return Program.need(n[1])
        if k == 'cond':
            # three live values: the k-th computed holds k registers below it
            return max(Program.need(c) + i
                       for i, c in enumerate(_select_order(n)))
        if k == 'powi':
            m = n[2]
            na = Program.need(n[1])
            return na if m & (m - 1) == 0 else max(na, 2)
        la, lb = Program.need(n[1]), Program.need(n[2])
        return la + 1 if la == lb else max(la, lb)

    def _gen(self, n, base):
        k = n[0]
        if k == 'num':
            self._emit('const', base, self._const(('num', n[1])))
        elif k == 'const':
            self._emit('const', base, self._const((n[1], n[2])))
        elif k == 'x':
            self._emit('coord', base, n[1])
        elif k == 'n':
            self._emit('normal', base, n[1])
        elif k == 'reg':
            self._emit('mov', base, n[1])
        elif k == 'field' and self.field_sides is not None:
            self._gen_side(n, 0, base)      # (unrestricted: evaluated on '+')
        elif k == 'field':
            self._emit('field', base, self._slot(
                self.fields, (n[1], n[2]), MAX_FIELDS, 'field components'),
                n[3])
        elif k == 'expr':
            self._emit('expr', base, self._slot(
                self.exprs, (n[1], n[2]), MAX_EXPRESSIONS,
                'Expression components'))
        elif k == 'cell':
            self._emit('cell', base, n[2])
        elif k == 'farea':
            self._emit('facet_len', base)
        elif k == 'side':
            self._gen_side(n[1], n[2], base)
        elif k in UNARY + UNARY_EXT:
            self._gen(n[1], base)
            self._emit(k, base, base)
        elif k == 'cond':
            # R[dst] = R[a] != 0 ? R[b] : R[dst]: dst holds the else-value
            order = _select_order(n)
            for i, c in enumerate(order):
                self._gen(c, base + i)
            rc, rt, rf = [base + [j for j in range(3) if order[j] is c][0]
                          for c in n[1:]]
            self._emit('select', rf, rc, rt)
            if rf != base:
                self._emit('mov', base, rf)
        elif k == 'powi':
            m = n[2]
            self._gen(n[1], base)
            if m & (m - 1) == 0:            # a power of two: square in place
                while m > 1:
                    self._emit('mul', base, base, base)
                    m >>= 1
            else:                           # left-to-right binary powering
                self._emit('mov', base + 1, base)
                for bit in bin(m)[3:]:
                    self._emit('mul', base + 1, base + 1, base + 1)
                    if bit == '1':
                        self._emit('mul', base + 1, base + 1, base)
                self._emit('mov', base, base + 1)
        else:
            a, b = n[1], n[2]
            if k in ('gt', 'ge'):           # a > b is b < a
                k, a, b = {'gt': 'lt', 'ge': 'le'}[k], b, a
            if self.need(a) >= self.need(b):
                self._gen(a, base)
                self._gen(b, base + 1)
                self._emit(k, base, base, base + 1)
            else:
                self._gen(b, base)
                self._gen(a, base + 1)
                self._emit(k, base, base + 1, base)

    def _gen_side(self, leaf, s, base):
        '''A leaf restricted to side s: the instruction of the leaf with the
        side bit in its operand; a field component takes the slot of its
        (Function, component, side).'''
        k = leaf[0]
        if k == 'field':
            for slot, (key, side) in enumerate(zip(self.fields,
                                                   self.field_sides)):
                if key[0] is leaf[1] and key[1] == leaf[2] and side == s:
                    break
            else:
                if len(self.fields) == MAX_FIELDS:
                    raise ProgramLimit(
                        'the integrand needs more than %d field components '
                        "(u('+') and u('-') are two): the limit is %d"
                        % (MAX_FIELDS, MAX_FIELDS))
                slot = len(self.fields)
                self.fields.append((leaf[1], leaf[2]))
                self.field_sides.append(s)
            self._emit('field', base, slot, leaf[3] | SIDE_BIT['field'] * s)
        elif k == 'n':
            self._emit('normal', base, leaf[1] | SIDE_BIT['normal'] * s)
        elif k == 'cell':
            self._emit('cell', base, leaf[2] | SIDE_BIT['cell'] * s)
        else:
            raise ValueError('%s cannot be restricted' % _leaf_name(leaf))

    def constant_values(self):
        '''The constants' current values (Constants may be re-assigned
        between calls: they travel with every launch).'''
        out = []
        for k in self.consts:
            if isinstance(k[0], str):
                out.append(k[1])
            else:
                out.append(float(k[0].values()[k[1]]))
        return out


def argument_program(table, rank, facet=False):
    '''The Program of a coefficient table (argument_table): rank 2, slot
    3 b + a of 9; rank 1, slot b of 3; absent terms have no instruction.
    facet: the table of a ds part (the normal exists).'''
    if rank == 2:
        items = [(3 * b + a, table[b][a]) for b in range(3) for a in range(3)]
    else:
        items = list(enumerate(table))
    items = [(k, t) for k, t in items if t is not None]
    return Program([t for _, t in items], slots=[k for k, _ in items],
                   nout=9 if rank == 2 else 3, facet=facet)


def _select_order(n):
    '''The order in which the condition and the two branches of ('cond', c,
    t, f) are computed into registers base, base + 1, base + 2: the largest
    register need first (else-value, condition, then-value among equals).'''
    return sorted((n[3], n[1], n[2]), key=lambda c: -Program.need(c))


def _count(n):
    '''Instructions Program._gen emits for the tree n.'''
    k = n[0]
    if k in UNARY + UNARY_EXT:
        return _count(n[1]) + 1
    if k == 'cond':
        return sum(_count(c) for c in n[1:]) + (
            1 if _select_order(n)[0] is n[3] else 2)
    if k == 'powi':
        m = n[2]
        if m & (m - 1) == 0:
            return _count(n[1]) + m.bit_length() - 1
        return _count(n[1]) + 2 + sum(2 if b == '1' else 1 for b in bin(m)[3:])
    if k in BINARY + BINARY_EXT + COMPARE:
        return _count(n[1]) + _count(n[2]) + 1
    return 1


def _subtrees(n, found):
    '''The non-leaf subtrees of n, into the set `found`.'''
    if n[0] in NONLEAF:
        found.add(n)
        for c in n[1:]:
            if isinstance(c, tuple):
                _subtrees(c, found)
    return found


def _substitute(n, old, new):
    if n == old:
        return new
    if n[0] in NONLEAF:
        return (n[0],) + tuple(_substitute(c, old, new)
                               if isinstance(c, tuple) else c for c in n[1:])
    return n


def _occurrences(n, c):
    """How often the subtree c occurs in the tree n."""
    if n == c:
        return 1
    if n[0] in NONLEAF:
        return sum(_occurrences(m, c) for m in n[1:] if isinstance(m, tuple))
    return 0


def share_subtrees(trees, within=False):
    '''Common-subtree sharing for the output trees of one program: (shared,
    trees) with shared = [(register, tree)] in the order to compute them and
    the output trees rewritten to read them through ('reg', r) leaves.
    Candidates are the structurally equal (==; objects inside by identity)
    non-leaf subtrees that occur in two or more trees (within=True: two or
    more times, in one tree or several), the largest first; each taken one
    gets the highest free register; one is taken where that saves
    instructions and still leaves every output tree, and every shared
    subtree, its Sethi-Ullman need below the reserved registers.'''
    trees = list(trees)
    seen = {}
    order = []
    for t in trees:
        for c in _subtrees(t, set()):
            if c not in seen:
                seen[c] = 0
                order.append(c)
            seen[c] += _occurrences(t, c) if within else 1
    cands = [c for c in order if seen[c] >= 2]
    # (largest first; ties by the instruction stream they would emit, which
    # is the same from run to run)
    cands.sort(key=lambda c: (-_count(c), repr(_strip(c))))
    defs = []           # (register, original tree, tree as it is computed)
    for c in cands:
        users = [t for t in trees + [d[2] for d in defs]
                 if c in _subtrees(t, set())]
        m = sum(_occurrences(t, c) for t in users) if within else len(users)
        if m < 2 or _count(c) + 1 + m >= m * _count(c):
            continue
        r = REGISTERS - 1 - len(defs)
        leaf = ('reg', r)
        new_trees = [_substitute(t, c, leaf) for t in trees]
        new_defs = [(d[0], d[1], _substitute(d[2], c, leaf)) for d in defs] \
            + [(r, c, c)]
        free = REGISTERS - len(new_defs)
        if all(Program.need(t) <= free for t in new_trees) and all(
                Program.need(d[2]) <= free for d in new_defs):
            trees, defs = new_trees, new_defs
    # (a subtree of a larger shared one was taken after it: compute it first)
    defs.sort(key=lambda d: _count(d[1]))
    return [(d[0], d[2]) for d in defs], trees


def compile_trees(trees, **kwargs):
    '''Program(trees, ...) as it always was where that fits the limits of
    flow_form; else with the subtrees that repeat, inside one tree or across
    them, computed once (share_subtrees, within=True) -- xi(Pe) names Pe five
    times.  The first ValueError where sharing does not help.'''
    trees = list(trees)
    try:
        return Program(trees, **kwargs)
    except ProgramLimit as e:
        shared, new = share_subtrees(trees, within=True)
        if not shared:
            raise
        try:
            return Program(new, shared=shared, **kwargs)
        except ProgramLimit:
            raise e


def _strip(n):
    '''The tree with the objects inside replaced by their kinds (sort key).'''
    return tuple(_strip(c) if isinstance(c, tuple) else
                 (c if isinstance(c, (str, int, float)) else type(c).__name__)
                 for c in n)


def newton_program(tableJ, tableF, share=True):
    '''ONE Program for the coefficient tables of a Jacobian (rank 2) and of a
    residual (rank 1) at the same state: slot 3 b + a of the first, 9 + b of
    the second, nout = 12.  The subtrees the two tables share (u, grad u and
    the nonlinearity appear in both) are computed once (share_subtrees;
    share=False: every tree on its own, as argument_program compiles them).
    ValueError where the combined program exceeds a limit of flow_form: the
    caller then runs the two programs one after the other.'''
    items = [(3 * b + a, tableJ[b][a]) for b in range(3) for a in range(3)]
    items += [(9 + b, tableF[b]) for b in range(3)]
    items = [(k, t) for k, t in items if t is not None]
    trees = [t for _, t in items]
    shared = ()
    if share:
        shared, trees = share_subtrees(trees)
    return Program(trees, slots=[k for k, _ in items], nout=NEWTON_SLOTS,
                   shared=shared)


def argument_programs(table, rank, facet=False):
    '''The coefficient table as a list of Programs whose cell tensors add up
    to the form's: [argument_program(table, rank)] where that fits the
    limits of flow_form; else the slots are dealt, in order, to as few
    programs as fit (each with its common subtrees computed once, as
    newton_program's), and the caller sums what they assemble.  ValueError
    where one coefficient alone exceeds a limit.  facet: the table of a ds
    part, whose coefficients may read the normal.'''
    try:
        return [argument_program(table, rank, facet)]
    except ValueError:
        pass
    if rank == 2:
        items = [(3 * b + a, table[b][a]) for b in range(3) for a in range(3)]
    else:
        items = list(enumerate(table))
    items = [(k, t) for k, t in items if t is not None]
    nout = 9 if rank == 2 else 3

    def build(chunk):
        try:
            shared, trees = share_subtrees([t for _, t in chunk])
            return Program(trees, slots=[k for k, _ in chunk], nout=nout,
                           shared=shared, facet=facet)
        except ProgramLimit:
            # (subtrees that repeat inside one coefficient, too)
            return compile_trees([t for _, t in chunk],
                                 slots=[k for k, _ in chunk], nout=nout,
                                 facet=facet)

    progs, chunk = [], []
    for item in items:
        try:
            prog = build(chunk + [item])
            chunk.append(item)
        except ValueError:
            if not chunk:
                raise
            progs.append(held)
            chunk = [item]
            prog = build(chunk)         # (ValueError: one slot is too long)
        held = prog
    progs.append(held)
    return progs


def depends_on(n, u):
    '''Whether the scalar tree n reads the Function u -- itself, or through
    a view u.split() / u.sub(i) of a Function of a Taylor-Hood space.'''
    if n[0] == 'field':
        own = getattr(n[1], 'mixed_owner', None)
        return n[1] is u or (own is not None and own[0] is u)
    return n[0] in NONLEAF and any(
        depends_on(c, u) for c in n[1:] if isinstance(c, tuple))


def form_mesh(expr, mesh=None):
    '''The mesh an expression lives on (ValueError if it has none).'''
    m = _join_mesh(expr.mesh, mesh)
    if m is None:
        raise ValueError('the integrand carries no mesh: integrate over '
                         'dx(mesh) or ds(mesh)')
    return m
