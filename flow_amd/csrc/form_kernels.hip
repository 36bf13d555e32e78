// Integrals of UFL-style expressions of fields (flow_amd/fem/forms.py): one
// kernel family that runs a host-compiled register program (include/
// flow_hip.h, flow_form) at every quadrature point of every cell.
//
//   functional   assemble(f*dx): per-cell integrals to scratch[cell], then
//                <= kRedBlocks block partials -> one finishing block
//                (sum_partials_host), fixed order, no fp atomics: two calls
//                give the same bits;
//   facets       assemble(f*ds): one lane per listed exterior facet, the
//                per-facet integrals to scratch[k], then the same reduction;
//   load vector  b_i = int f phi_i (project): per-cell values to
//                scratch[(o*nloc + i)*nc + c], then the gather of
//                assembly_kernels.hip, as flow_assemble_source does;
//   points       u(x), Probes: one lane per located point, the program at
//                its barycentric coordinates (flow_locate_points finds the
//                cell: the bucket grid's candidates in ascending order, the
//                first cell that holds the point).
//
// One thread per cell, a loop over the rule's points, the program inside it.
// The program and the constants are kernel arguments: every lane reads the
// same instruction (scalar loads, wave-uniform dispatch, no divergence).  The
// eight registers and the field slots are NAMED values behind switches and
// unrolled compile-time loops -- a register file indexed at run time would
// live in scratch memory.  Scratch stays at 0 bytes per lane.
#include <cmath>
#include <type_traits>

#include "fem_device.h"

namespace flow {

// flow_locate_points: a point lies in a cell when all three barycentric
// coordinates are >= this (include/flow_hip.h)
constexpr double kPointTol = -1.0e-12;

struct FormRegs {
  double r0, r1, r2, r3, r4, r5, r6, r7;
};

__device__ __forceinline__ double reg_get(const FormRegs& R, int i) {
  switch (i) {
    case 0: return R.r0;
    case 1: return R.r1;
    case 2: return R.r2;
    case 3: return R.r3;
    case 4: return R.r4;
    case 5: return R.r5;
    case 6: return R.r6;
    default: return R.r7;
  }
}

__device__ __forceinline__ void reg_set(FormRegs& R, int i, double v) {
  switch (i) {
    case 0: R.r0 = v; break;
    case 1: R.r1 = v; break;
    case 2: R.r2 = v; break;
    case 3: R.r3 = v; break;
    case 4: R.r4 = v; break;
    case 5: R.r5 = v; break;
    case 6: R.r6 = v; break;
    default: R.r7 = v; break;
  }
}

// sin (cos = false) or cos of x.  The library's sin / cos carry a reduction
// for arguments of any size whose tables and constants cost the kernel ~30
// scalar registers and made it spill them; the arguments of a form are
// coordinates, times and field values.  Here: x = n pi/2 + r, |r| <= pi/4,
// with a two-part pi/2 through FMAs (accurate while n pi/2 stays well inside
// the double range of exact multiples, |x| < ~1e9), then the fdlibm minimax
// polynomials of sin and cos on [-pi/4, pi/4] (error < 1 ulp there).
__device__ __forceinline__ double form_sincos(double x, bool want_cos) {
  const double n = rint(x * 0.63661977236758134308);          // 2/pi
  double r = fma(-n, 1.5707963267948965580, x);               // pi/2, high part
  r = fma(-n, 6.1232339957367658e-17, r);                     // pi/2 - high part
  const double z = r * r;
  const double sp = -1.66666666666666324348e-01 +
      z * (8.33333333332248946124e-03 +
      z * (-1.98412698298579493134e-04 +
      z * (2.75573137070700676789e-06 +
      z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10))));
  const double cp = 4.16666666666666019037e-02 +
      z * (-1.38888888888741095749e-03 +
      z * (2.48015872894767294178e-05 +
      z * (-2.75573143513906633035e-07 +
      z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))));
  const double s = r + r * z * sp;
  const double c = 1.0 - 0.5 * z + z * z * cp;
  // quadrant of x (+1 for cos: cos x = sin(x + pi/2))
  const double m = n + (want_cos ? 1.0 : 0.0);
  const int quad = static_cast<int>(m - 4.0 * floor(m * 0.25));
  const double v = (quad & 1) ? c : s;
  return (quad & 2) ? -v : v;
}

// value (d = 0) or d/dx, d/dy (d = 1, 2) of field slot s at barycentric L
template <int NF>
__device__ __forceinline__ double field_at(const flow_form& F,
                                           const double (&U)[NF][6], int s,
                                           int d, const double L[3],
                                           const Geom& g) {
  double v = 0.0;
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    if (k != s) continue;
    const double* u = U[k];
    if (F.field_deg[k] == 1) {
      if (d == 0) {
        v = u[0] * L[0] + u[1] * L[1] + u[2] * L[2];
      } else {
        const int e = d - 1;
        v = u[0] * (e == 0 ? g.gl[0][0] : g.gl[0][1]) +
            u[1] * (e == 0 ? g.gl[1][0] : g.gl[1][1]) +
            u[2] * (e == 0 ? g.gl[2][0] : g.gl[2][1]);
      }
    } else {
      if (d == 0) {
        v = eval_at<2>(u, L);
      } else {
        double gur[3];
        ref_gradient<2>(u, L, gur);
        const int e = d - 1;
        v = gur[0] * (e == 0 ? g.gl[0][0] : g.gl[0][1]) +
            gur[1] * (e == 0 ? g.gl[1][0] : g.gl[1][1]) +
            gur[2] * (e == 0 ? g.gl[2][0] : g.gl[2][1]);
      }
    }
  }
  return v;
}

// The program at one point: L its barycentric coordinates on cell c, row its
// row of the rule (and of the Expression tables).  FACET: the point lies on a
// facet whose outward unit normal is (n0, n1); the cell kernels pass
// FACET = false, their programs never hold NORMAL (check_form).
//
// OUT receives the `out` instructions: FormOut2 for the functionals, load
// vectors and points, FormSlots<9> / <3> for the coefficient tables of rank-2
// / rank-1 forms, <12> for both tables of a Newton pass.  Like the registers,
// the outputs are named values.
struct FormOut2 {
  double& out0;
  double& out1;
  __device__ __forceinline__ void set(int b, double r) {
    out0 = b == 0 ? r : out0;
    out1 = b == 0 ? out1 : r;
  }
};

template <int N>
struct FormSlots {
  double v[N];
  // (a wave-uniform switch, as reg_set: N selects would hold N lane masks in
  // scalar registers at once)
  __device__ __forceinline__ void set(int b, double r) {
    switch (b) {
      case 0: v[0] = r; break;
      case 1: v[1 < N ? 1 : 0] = r; break;
      case 2: v[2 < N ? 2 : 0] = r; break;
      case 3: v[3 < N ? 3 : 0] = r; break;
      case 4: v[4 < N ? 4 : 0] = r; break;
      case 5: v[5 < N ? 5 : 0] = r; break;
      case 6: v[6 < N ? 6 : 0] = r; break;
      case 7: v[7 < N ? 7 : 0] = r; break;
      // (N = 12, the set of form_newton_kernel: 3 b + a of the Jacobian's
      // table, then 9 + b of the residual's.  In a smaller set these cases
      // store where the default does, and fold into it: the switch of
      // FormSlots<9> / <3> is the one it was before N = 12 existed)
      case 8: v[8 < N ? 8 : N - 1] = r; break;
      case 9: v[9 < N ? 9 : N - 1] = r; break;
      case 10: v[10 < N ? 10 : N - 1] = r; break;
      default: v[N - 1] = r; break;
    }
  }
};

// tanh x from e = exp(-2|x|), which the interpreter's one exp computed: for
// |x| >= 1/2, (1 - e) / (1 + e) with e <= 0.37 (no cancellation; e -> 0 gives
// +-1, never inf/inf); below, x P(x^2) / Q(x^2), the [7/6] Pade approximant
// from the continued fraction x / (1 + x^2 / (3 + x^2 / (5 + ...))) (error <
// 1e-17 relative there, exact to first order at 0).  One division.
__device__ __forceinline__ double form_tanh(double x, double e) {
  const double z = x * x;
  const bool small = z < 0.25;
  const double pn = x * (135135.0 + z * (17325.0 + z * (378.0 + z)));
  const double pd = 135135.0 + z * (62370.0 + z * (3150.0 + z * 28.0));
  return (small ? pn : copysign(1.0 - e, x)) / (small ? pd : 1.0 + e);
}

// The extended opcodes (FLOW_FORM_OP_LT and up) but tanh.  They are compiled
// into instances of their own (EXT = true, chosen on the host where the
// program holds one): the instances every other program runs keep the
// registers and the occupancy they had.
__device__ __forceinline__ double form_ext_op(int op, int a, double ra, double rb,
                                              double rd, const double X[3],
                                              const double Y[3], const Geom& g) {
  switch (op) {
    case FLOW_FORM_OP_LT: return ra < rb ? 1.0 : 0.0;
    case FLOW_FORM_OP_LE: return ra <= rb ? 1.0 : 0.0;
    case FLOW_FORM_OP_EQ: return ra == rb ? 1.0 : 0.0;
    case FLOW_FORM_OP_NE: return ra != rb ? 1.0 : 0.0;
    // a real select: the value not taken is never combined with the result
    case FLOW_FORM_OP_SELECT: return ra != 0.0 ? rb : rd;
    // (fmin / fmax return the other operand where one is NaN; sign returns
    // +-0 and NaN as they are: include/flow_hip.h)
    case FLOW_FORM_OP_MIN: return fmin(ra, rb);
    case FLOW_FORM_OP_MAX: return fmax(ra, rb);
    case FLOW_FORM_OP_SIGN: return ra > 0.0 ? 1.0 : (ra < 0.0 ? -1.0 : ra);
    default: {   // FLOW_FORM_OP_CELL
      // from the vertex coordinates the lane holds (no load): squared edge
      // lengths, then |T| = |det J| / 2, the circumradius abc / (4 |T|) or
      // the largest vertex distance
      const double e0 = (X[1] - X[0]) * (X[1] - X[0]) + (Y[1] - Y[0]) * (Y[1] - Y[0]);
      const double e1 = (X[2] - X[1]) * (X[2] - X[1]) + (Y[2] - Y[1]) * (Y[2] - Y[1]);
      const double e2 = (X[0] - X[2]) * (X[0] - X[2]) + (Y[0] - Y[2]) * (Y[0] - Y[2]);
      const double s = sqrt(a == 1 ? e0 * e1 * e2 : fmax(e0, fmax(e1, e2)));
      return a == 0 ? 0.5 * g.adet : (a == 1 ? s / (2.0 * g.adet) : s);
    }
  }
}

// The '-' cell of an interior facet, next to the '+' cell that the other
// arguments of form_point_n describe (TWO = true, form_interior_facet_kernel):
// geometry, vertex coordinates, the point's barycentric coordinates there, the
// cell's own outward normal and the facet's length.
struct FormMinus {
  Geom g;
  double X[3], Y[3];
  double L[3];
  double n0, n1;
  double len;
};

// g of the side an instruction names.  Selects of values, entry by entry: the
// side is wave-uniform, and a selected ADDRESS would be a run-time index
// (facet_frame)
__device__ __forceinline__ Geom side_geom(const Geom& p, const Geom& m, bool minus) {
  Geom g;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    g.gl[i][0] = minus ? +m.gl[i][0] : +p.gl[i][0];
    g.gl[i][1] = minus ? +m.gl[i][1] : +p.gl[i][1];
  }
  g.adet = minus ? +m.adet : +p.adet;
  return g;
}

// TWO: the program of an interior facet.  FIELD, NORMAL and CELL carry a side
// bit (FLOW_FORM_SIDE_*): set, the leaf is evaluated on the '-' cell *M, whose
// field slots the kernel loaded from that cell; FACET_LEN exists.  Every other
// instance passes TWO = false and compiles to what it was.
template <int NF, bool FACET, bool EXT, bool TWO = false, class OUT>
__device__ __forceinline__ void form_point_n(const flow_form& F,
                                             const double (&U)[NF > 0 ? NF : 1][6],
                                             const double X[3], const double Y[3],
                                             const Geom& g, const double L[3], int row,
                                             int nc, int c, double n0, double n1,
                                             OUT& out, const FormMinus* M = nullptr) {
  FormRegs R = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int pc = 0; pc < F.nprog; ++pc) {
    int op = F.prog[4 * pc];
    const int dst = F.prog[4 * pc + 1];
    const int a = F.prog[4 * pc + 2], b = F.prog[4 * pc + 3];
    double v;
    bool tanh_op = false;
    if constexpr (TWO) {
      if (op == FLOW_FORM_OP_FACET_LEN) {
        reg_set(R, dst, M->len);
        continue;
      }
      if (op == FLOW_FORM_OP_FIELD) {
        const bool minus = (b & FLOW_FORM_SIDE_FIELD) != 0;
        const Geom gs = side_geom(g, M->g, minus);
        const double Ls[3] = {minus ? +M->L[0] : +L[0], minus ? +M->L[1] : +L[1],
                              minus ? +M->L[2] : +L[2]};
        if constexpr (NF > 0) v = field_at<NF>(F, U, a, b & 3, Ls, gs);
        else v = 0.0;
        reg_set(R, dst, v);
        continue;
      }
      if (op == FLOW_FORM_OP_NORMAL) {
        const bool minus = (a & FLOW_FORM_SIDE_NORMAL) != 0;
        const double m0 = minus ? +M->n0 : +n0, m1 = minus ? +M->n1 : +n1;
        reg_set(R, dst, (a & 1) == 0 ? m0 : m1);
        continue;
      }
      if (EXT && op == FLOW_FORM_OP_CELL) {
        const bool minus = (a & FLOW_FORM_SIDE_CELL) != 0;
        const Geom gs = side_geom(g, M->g, minus);
        double Xs[3], Ys[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          Xs[i] = minus ? +M->X[i] : +X[i];
          Ys[i] = minus ? +M->Y[i] : +Y[i];
        }
        reg_set(R, dst, form_ext_op(op, a & 3, 0.0, 0.0, 0.0, Xs, Ys, gs));
        continue;
      }
    }
    if constexpr (EXT) {
      // tanh goes through the exp below; the others have a switch of their own
      tanh_op = op == FLOW_FORM_OP_TANH;
      if (tanh_op) {
        op = FLOW_FORM_OP_EXP;
      } else if (op >= FLOW_FORM_OP_LT) {
        const bool two = op <= FLOW_FORM_OP_MAX;
        reg_set(R, dst,
                form_ext_op(op, a, op == FLOW_FORM_OP_CELL ? 0.0 : reg_get(R, a),
                            two ? reg_get(R, b) : 0.0,
                            op == FLOW_FORM_OP_SELECT ? reg_get(R, dst) : 0.0, X, Y, g));
        continue;
      }
    }
    switch (op) {
      case FLOW_FORM_OP_CONST: v = F.consts[a]; break;
      case FLOW_FORM_OP_COORD: {
        const double* P = a == 0 ? X : Y;
        v = P[0] * L[0] + P[1] * L[1] + P[2] * L[2];
        break;
      }
      case FLOW_FORM_OP_FIELD:
        // (TWO: taken above, with the side's geometry)
        if constexpr (NF > 0 && !TWO) v = field_at<NF>(F, U, a, b, L, g);
        else v = 0.0;
        break;
      case FLOW_FORM_OP_EXPR: {
        const int nl = F.expr_nl[a];
        const double* tab = F.tables + F.expr_table[a] + row * nl;
        const double* e = F.expr[a];
        double s = 0.0;
        for (int l = 0; l < nl; ++l) s += e[static_cast<size_t>(l) * nc + c] * tab[l];
        v = s;
        break;
      }
      case FLOW_FORM_OP_NORMAL:
        if constexpr (FACET) v = a == 0 ? n0 : n1;
        else v = 0.0;
        break;
      case FLOW_FORM_OP_MOV: v = reg_get(R, a); break;
      case FLOW_FORM_OP_ADD: v = reg_get(R, a) + reg_get(R, b); break;
      case FLOW_FORM_OP_SUB: v = reg_get(R, a) - reg_get(R, b); break;
      case FLOW_FORM_OP_MUL: v = reg_get(R, a) * reg_get(R, b); break;
      case FLOW_FORM_OP_DIV: v = reg_get(R, a) / reg_get(R, b); break;
      case FLOW_FORM_OP_NEG: v = -reg_get(R, a); break;
      case FLOW_FORM_OP_ABS: v = fabs(reg_get(R, a)); break;
      case FLOW_FORM_OP_SQRT: v = sqrt(reg_get(R, a)); break;
      // one log and one exp serve ln, exp and pow (a^b = exp(b ln a); the
      // host sends integer exponents as multiplies and divisions, so pow
      // only meets the exponents for which a < 0 is undefined anyway):
      // every library routine is inlined once, which keeps the registers down
      case FLOW_FORM_OP_POW:
      case FLOW_FORM_OP_EXP:
      case FLOW_FORM_OP_LN: {
        double t = reg_get(R, a);
        if constexpr (EXT) {
          if (tanh_op) t = -2.0 * fabs(t);
        }
        if (op != FLOW_FORM_OP_EXP) t = log(t);
        if (op == FLOW_FORM_OP_POW) t *= reg_get(R, b);
        v = op == FLOW_FORM_OP_LN ? t : exp(t);
        if constexpr (EXT) {
          if (tanh_op) v = form_tanh(reg_get(R, a), v);
        }
        break;
      }
      case FLOW_FORM_OP_SIN:
      case FLOW_FORM_OP_COS: v = form_sincos(reg_get(R, a), op == FLOW_FORM_OP_COS); break;
      default: {   // FLOW_FORM_OP_OUT
        out.set(b, reg_get(R, a));
        continue;
      }
    }
    reg_set(R, dst, v);
  }
}

// the two-output program of the functionals, load vectors and points
template <int NF, bool FACET, bool EXT>
__device__ __forceinline__ void form_point(const flow_form& F,
                                           const double (&U)[NF > 0 ? NF : 1][6],
                                           const double X[3], const double Y[3],
                                           const Geom& g, const double L[3], int row,
                                           int nc, int c, double n0, double n1,
                                           double& out0, double& out1) {
  FormOut2 out = {out0, out1};
  form_point_n<NF, FACET, EXT>(F, U, X, Y, g, L, row, nc, c, n0, n1, out);
}

// the local values of the form's fields on cell c
template <int NF>
__device__ __forceinline__ void load_form_fields(const flow_form& F, int nc, int c,
                                                 double (&U)[NF > 0 ? NF : 1][6]) {
  if constexpr (NF > 0) {
    bool p1 = false, p2 = false;
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      p1 = p1 || F.field_deg[k] == 1;
      p2 = p2 || F.field_deg[k] == 2;
    }
    int d1[3] = {0, 0, 0}, d2[6] = {0, 0, 0, 0, 0, 0};
    if (p1) {
#pragma unroll
      for (int i = 0; i < 3; ++i) d1[i] = F.cell_dofs[0][i * nc + c];
    }
    if (p2) {
#pragma unroll
      for (int i = 0; i < 6; ++i) d2[i] = F.cell_dofs[1][i * nc + c];
    }
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      const double* f = F.field[k];
      if (F.field_deg[k] == 1) {
#pragma unroll
        for (int i = 0; i < 3; ++i) U[k][i] = f[d1[i]];
#pragma unroll
        for (int i = 3; i < 6; ++i) U[k][i] = 0.0;
      } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) U[k][i] = f[d2[i]];
      }
    }
  }
}

// What a lane holds of its cell while the program runs: the geometry, the
// vertex coordinates and the local values of the form's fields.  Every form
// kernel starts with load_form_cell.
template <int NF>
struct FormCell {
  Geom g;
  double X[3], Y[3];
  double U[NF > 0 ? NF : 1][6];
};

template <int NF>
__device__ __forceinline__ void load_form_cell(const flow_form& F, int nc,
                                               const double* xy, int c,
                                               FormCell<NF>& C) {
  C.g = load_geom(xy, nc, c);
#pragma unroll
  for (int v = 0; v < 3; ++v) C.X[v] = xy[v * nc + c];
#pragma unroll
  for (int v = 0; v < 3; ++v) C.Y[v] = xy[(3 + v) * nc + c];
  load_form_fields<NF>(F, nc, c, C.U);
}

// Outward unit normal (n0, n1) and length of local facet lf of a cell:
// -grad(lambda_lf) / |grad lambda_lf| and |det J| |grad lambda_lf|.
struct FacetFrame {
  double n0, n1, len;
};

__device__ __forceinline__ FacetFrame facet_frame(const Geom& g, int lf) {
  // (selects, not g.gl[lf]: a run-time index would put g in scratch memory.
  // Selects of VALUES loaded beforehand: g is a reference here, and loads
  // under the branches of a conditional are merged into one load from a
  // selected address, which is a run-time index again.  The unary + makes
  // each operand a value: a conditional between two named doubles is itself
  // an lvalue, that is, a selected address once more)
  const double x0 = g.gl[0][0], x1 = g.gl[1][0], x2 = g.gl[2][0];
  const double y0 = g.gl[0][1], y1 = g.gl[1][1], y2 = g.gl[2][1];
  const double gx = lf == 0 ? +x0 : (lf == 1 ? +x1 : +x2);
  const double gy = lf == 0 ? +y0 : (lf == 1 ? +y1 : +y2);
  const double gn = sqrt(gx * gx + gy * gy);
  return {-gx / gn, -gy / gn, g.adet * gn};
}

// Runs the program at every point of the rule on cell c.  TD = 0: returns
// sum_q w_q |det J| out_0(x_q); TD = 1, 2: acc[o][i] += w_q |det J| out_o phi_i.
template <int NF, int TD, bool EXT>
__device__ __forceinline__ double form_cell(const flow_form& F, int nc,
                                            const double* __restrict__ xy, int c,
                                            double (&acc)[2][6]) {
  FormCell<NF> C;
  load_form_cell<NF>(F, nc, xy, c, C);
  const Geom& g = C.g;
  double total = 0.0;
  for (int q = 0; q < F.nq; ++q) {
    const double xi = F.rule[3 * q], eta = F.rule[3 * q + 1];
    const double w = F.rule[3 * q + 2] * g.adet;
    const double L[3] = {1.0 - xi - eta, xi, eta};
    double out0 = 0.0, out1 = 0.0;
    form_point<NF, false, EXT>(F, C.U, C.X, C.Y, g, L, q, nc, c, 0.0, 0.0, out0, out1);
    if constexpr (TD == 0) {
      total += w * out0;
    } else {
      const double s0 = w * out0, s1 = w * out1;
      if constexpr (TD == 1) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          acc[0][i] += s0 * L[i];
          acc[1][i] += s1 * L[i];
        }
      } else {
        double phi[6], dphi[6][3];
        basis<2>(L, phi, dphi);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          acc[0][i] += s0 * phi[i];
          acc[1][i] += s1 * phi[i];
        }
      }
    }
  }
  return total;
}

// The integral of output 0 over local facet lf of cell c: the rule's rows
// lf*nq .. lf*nq + nq - 1 (reference coordinates on that facet, weights
// summing to 1) scaled by the facet's length |det J| |grad lambda_lf|; the
// outward unit normal is -grad(lambda_lf) / |grad lambda_lf|.
template <int NF, bool EXT>
__device__ __forceinline__ double form_facet(const flow_form& F, int nc,
                                             const double* __restrict__ xy, int c,
                                             int lf) {
  FormCell<NF> C;
  load_form_cell<NF>(F, nc, xy, c, C);
  const FacetFrame f = facet_frame(C.g, lf);
  double total = 0.0;
  for (int j = 0; j < F.nq; ++j) {
    const int row = lf * F.nq + j;
    const double xi = F.rule[3 * row], eta = F.rule[3 * row + 1];
    const double L[3] = {1.0 - xi - eta, xi, eta};
    double out0 = 0.0, out1 = 0.0;
    form_point<NF, true, EXT>(F, C.U, C.X, C.Y, C.g, L, row, nc, c, f.n0, f.n1, out0,
                              out1);
    total += F.rule[3 * row + 2] * f.len * out0;
  }
  return total;
}

// functional, stage 2: fixed-order sum of the per-cell integrals, one partial
// per block
__global__ __launch_bounds__(kBlock) void form_sum_kernel(
    int cb, int ce, const double* __restrict__ cellv, double* __restrict__ partials) {
  double s = 0.0;
  for (int c = cb + blockIdx.x * blockDim.x + threadIdx.x; c < ce;
       c += gridDim.x * blockDim.x)
    s += cellv[c];
  s = block_sum_once(s);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// one cell per lane.  TD = 0 (functional, stage 1): scratch[cell] = the
// cell's integral; TD = 1, 2 (load vector): [o][i][cell] contributions for
// the gather
template <int NF, int TD, bool EXT>
__global__ __launch_bounds__(kBlock) void form_cell_kernel(
    int nc, int cb, int ce, const double* __restrict__ xy, const flow_form F,
    double* __restrict__ scratch) {
  const int c = cb + blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ce) return;
  double acc[2][6];
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[o][i] = 0.0;
  const double total = form_cell<NF, TD, EXT>(F, nc, xy, c, acc);
  if constexpr (TD == 0) {
    scratch[c] = total;
    return;
  }
  constexpr int NL = TD == 1 ? 3 : 6;
#pragma unroll
  for (int i = 0; i < NL; ++i) scratch[static_cast<size_t>(i) * nc + c] = acc[0][i];
  if (F.nout == 2) {
#pragma unroll
    for (int i = 0; i < NL; ++i)
      scratch[static_cast<size_t>(NL + i) * nc + c] = acc[1][i];
  }
}

// one facet per lane: scratch[k] = the integral over facet k of the list
// (cell, local facet); a facet outside the mesh gives NaN, not a stray read
template <int NF, bool EXT>
__global__ __launch_bounds__(kBlock) void form_facet_kernel(
    int nc, int nfacets, const int* __restrict__ fcell,
    const int* __restrict__ flocal, const double* __restrict__ xy,
    const flow_form F, double* __restrict__ scratch) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nfacets) return;
  const int c = fcell[k], lf = flocal[k];
  if (c < 0 || c >= nc || lf < 0 || lf > 2) {
    scratch[k] = __builtin_nan("");
    return;
  }
  scratch[k] = form_facet<NF, EXT>(F, nc, xy, c, lf);
}

// Interior facets (assemble(f*dS), flow_form_interior_facet_*).  A lane holds
// TWO cells, but one U array: every (field, component, side) the program names
// is a field slot of its own, and slot k is loaded from the cell of its side
// (bit k of minus_slots set: the '-' cell).  Two FormCell<6> would be ~150
// VGPRs of nodal values alone.
template <int NF>
__device__ __forceinline__ void load_form_fields_sides(const flow_form& F, int nc, int cp,
                                                       int cm, int minus_slots,
                                                       double (&U)[NF > 0 ? NF : 1][6]) {
  if constexpr (NF > 0) {
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      const int c = ((minus_slots >> k) & 1) ? cm : cp;
      const double* f = F.field[k];
      if (F.field_deg[k] == 1) {
        const int* cd = F.cell_dofs[0];
#pragma unroll
        for (int i = 0; i < 3; ++i) U[k][i] = f[cd[i * nc + c]];
#pragma unroll
        for (int i = 3; i < 6; ++i) U[k][i] = 0.0;
      } else {
        const int* cd = F.cell_dofs[1];
#pragma unroll
        for (int i = 0; i < 6; ++i) U[k][i] = f[cd[i * nc + c]];
      }
    }
  }
}

// One interior facet per lane: out[k] = the integral over facet k of the
// list.  fplus / lplus: the '+' cell and the facet's local index in it;
// fother = (cell- << 3) | (local- << 1) | flip, packed as adapt.facet_table
// packs a neighbour.  The lane walks the rule's rows of local facet lplus on
// the '+' cell and scales by that cell's facet length.  On '-' the barycentric
// coordinates are zero at vertex local- and the '+' facet's pair on the facet's
// two vertices, swapped where flip is set (the first vertex of the facet in
// '-' is then the second in '+'); n('-') is the '-' cell's own facet_frame.  An
// entry outside the mesh gives NaN, not a stray read.
template <int NF, bool EXT>
__global__ __launch_bounds__(kBlock) void form_interior_facet_kernel(
    int nc, int nfacets, const int* __restrict__ fplus, const int* __restrict__ lplus,
    const int* __restrict__ fother, int minus_slots, const double* __restrict__ xy,
    const flow_form F, double* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nfacets) return;
  const int cp = fplus[k], lp = lplus[k], packed = fother[k];
  const int cm = packed >> 3, lm = (packed >> 1) & 3, flip = packed & 1;
  if (cp < 0 || cp >= nc || lp < 0 || lp > 2 || packed < 0 || cm >= nc || lm > 2) {
    out[k] = __builtin_nan("");
    return;
  }
  const Geom gp = load_geom(xy, nc, cp);
  FormMinus M;
  M.g = load_geom(xy, nc, cm);
  double X[3], Y[3];
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    X[v] = xy[v * nc + cp];
    Y[v] = xy[(3 + v) * nc + cp];
    M.X[v] = xy[v * nc + cm];
    M.Y[v] = xy[(3 + v) * nc + cm];
  }
  double U[NF > 0 ? NF : 1][6];
  load_form_fields_sides<NF>(F, nc, cp, cm, minus_slots, U);
  const FacetFrame fp = facet_frame(gp, lp);
  const FacetFrame fm = facet_frame(M.g, lm);
  M.n0 = fm.n0;
  M.n1 = fm.n1;
  M.len = fp.len;
  double total = 0.0;
  for (int j = 0; j < F.nq; ++j) {
    const int row = lp * F.nq + j;
    const double xi = F.rule[3 * row], eta = F.rule[3 * row + 1];
    const double L[3] = {1.0 - xi - eta, xi, eta};
    // the weights of the facet's first and second vertex in '+' ...
    const double a0 = lp == 0 ? +L[1] : +L[0], a1 = lp == 2 ? +L[1] : +L[2];
    // ... are those of its first and second vertex in '-', or the reverse
    const double b0 = flip ? a1 : a0, b1 = flip ? a0 : a1;
    M.L[0] = lm == 0 ? 0.0 : b0;
    M.L[1] = lm == 0 ? b0 : (lm == 1 ? 0.0 : b1);
    M.L[2] = lm == 2 ? 0.0 : b1;
    double out0 = 0.0, out1 = 0.0;
    FormOut2 o = {out0, out1};
    form_point_n<NF, true, EXT, true>(F, U, X, Y, gp, L, row, nc, cp, fp.n0, fp.n1, o, &M);
    total += F.rule[3 * row + 2] * fp.len * out0;
  }
  out[k] = total;
}

// flow_facet_cell_shares: one lane per cell, its three facets in the order
// 0, 1, 2; a position of -1 (a boundary facet, or one not selected) is skipped
__global__ __launch_bounds__(kBlock) void facet_cell_shares_kernel(
    int nc, int nfacets, const int* __restrict__ position,
    const double* __restrict__ values, double share, double* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int p = position[static_cast<size_t>(i) * nc + c];
    if (p >= 0 && p < nfacets) s += values[p];
  }
  out[c] = share * s;
}

// Wall distributions (flow_amd/fem/profile.py, flow_form_facet_values): one
// lane per (facet, sample) -- a boundary holds O(sqrt(N)) facets, the samples
// are the parallelism.  Lane (k, j) runs the program at row lf*m + j of the
// rule and writes output o to values[o*npoints + dest[k]*m + j'], j' = m-1-j
// where the curve runs against the facet's own direction (flip[k]): the
// samples land in arclength order.  Lane j == 0 of a facet goes on over the
// other rows and adds up the facet's integral with the arithmetic and the
// order of form_facet, to integrals[o*nfacets + dest[k]].  A facet outside
// the mesh gives NaN, a destination outside the list is not written.
template <int NF, bool EXT>
__global__ __launch_bounds__(kBlock) void form_facet_values_kernel(
    int nc, int nfacets, const int* __restrict__ fcell,
    const int* __restrict__ flocal, const int* __restrict__ fdest,
    const int* __restrict__ fflip, const double* __restrict__ xy,
    const flow_form F, double* __restrict__ values,
    double* __restrict__ integrals) {
  const int m = F.nq;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nfacets * m) return;
  const int k = i / m, j = i - k * m;
  const int d = fdest[k];
  if (d < 0 || d >= nfacets) return;
  const bool whole = integrals != nullptr && j == 0;
  const size_t np = static_cast<size_t>(nfacets) * m;
  double* const val = values + static_cast<size_t>(d) * m + (fflip[k] ? m - 1 - j : j);
  const int c = fcell[k], lf = flocal[k];
  if (c < 0 || c >= nc || lf < 0 || lf > 2) {
    const double bad = __builtin_nan("");
    val[0] = bad;
    if (F.nout == 2) val[np] = bad;
    if (whole) {
      integrals[d] = bad;
      if (F.nout == 2) integrals[static_cast<size_t>(nfacets) + d] = bad;
    }
    return;
  }
  FormCell<NF> C;
  load_form_cell<NF>(F, nc, xy, c, C);
  const FacetFrame f = facet_frame(C.g, lf);
  double total0 = 0.0, total1 = 0.0;
  // (one loop for the sample and the integral: the interpreter is inlined once)
  for (int q = j, qe = whole ? m : j + 1; q < qe; ++q) {
    const int row = lf * m + q;
    const double xi = F.rule[3 * row], eta = F.rule[3 * row + 1];
    const double L[3] = {1.0 - xi - eta, xi, eta};
    double out0 = 0.0, out1 = 0.0;
    form_point<NF, true, EXT>(F, C.U, C.X, C.Y, C.g, L, row, nc, c, f.n0, f.n1, out0,
                              out1);
    if (q == j) {
      val[0] = out0;
      if (F.nout == 2) val[np] = out1;
    }
    total0 += F.rule[3 * row + 2] * f.len * out0;
    total1 += F.rule[3 * row + 2] * f.len * out1;
  }
  if (whole) {
    integrals[d] = total0;
    if (F.nout == 2) integrals[static_cast<size_t>(nfacets) + d] = total1;
  }
}

// flow_profile_cumsum: one lane per (curve, row), the curve's facets added
// strictly left to right.  Boundaries hold thousands of facets, not millions,
// and the fixed order is the point: numpy.cumsum of the integrals gives the
// same bits.  The offsets travel with the launch.
struct ProfileCurves {
  int off[FLOW_PROFILE_CURVES_PER_LAUNCH + 1];
};

__global__ __launch_bounds__(kBlock) void profile_cumsum_kernel(
    int ncurves, const ProfileCurves C, int nrows, int nfacets,
    const double* __restrict__ integrals, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ncurves * nrows) return;
  const int c = i / nrows, r = i - c * nrows;
  // (selects over the argument array: the offsets stay in scalar registers)
  int b = 0, e = 0;
#pragma unroll
  for (int k = 0; k < FLOW_PROFILE_CURVES_PER_LAUNCH; ++k) {
    b = k == c ? C.off[k] : b;
    e = k == c ? C.off[k + 1] : e;
  }
  const double* src = integrals + static_cast<size_t>(r) * nfacets;
  double* dst = out + static_cast<size_t>(r) * nfacets;
  double s = 0.0;
  for (int k = b; k < e; ++k) {
    s += src[k];
    dst[k] = s;
  }
}

// The point of the mesh's cell c at barycentric (l0, l1, l2): the test of
// flow_locate_points.  Contraction stays off, so that the host's numpy
// evaluation of the same expressions (flow_amd/fem/points.py) gives the same
// bits: which cell a point on an edge belongs to is then decided alike.
__device__ __forceinline__ bool point_in_cell(const double* __restrict__ xy, int nc,
                                              int c, double px, double py,
                                              double& l0, double& l1, double& l2) {
#pragma clang fp contract(off)
  const double x0 = xy[0 * nc + c], x1 = xy[1 * nc + c], x2 = xy[2 * nc + c];
  const double y0 = xy[3 * nc + c], y1 = xy[4 * nc + c], y2 = xy[5 * nc + c];
  const double j00 = x1 - x0, j01 = x2 - x0, j10 = y1 - y0, j11 = y2 - y0;
  const double det = j00 * j11 - j01 * j10;
  const double dx = px - x0, dy = py - y0;
  l1 = (j11 * dx - j01 * dy) / det;
  l2 = (j00 * dy - j10 * dx) / det;
  l0 = 1.0 - l1 - l2;
  return l0 >= kPointTol && l1 >= kPointTol && l2 >= kPointTol;
}

// The cell of the point (px, py) and its barycentric coordinates there: its
// bucket's candidates in ascending cell order, the first that holds it (the
// lowest-index rule); -1 and NaN for a point in no cell.
__device__ __forceinline__ int locate_point(const double* __restrict__ xy, int nc,
                                            const flow_point_grid& G, double px,
                                            double py, double& l0, double& l1,
                                            double& l2) {
  // (clamped as doubles: a NaN or a far point never becomes an int out of
  // range; NaN fails every test below)
  double tx = (px - G.x0) * G.hx_inv, ty = (py - G.y0) * G.hy_inv;
  tx = tx >= 0.0 ? (tx <= G.nx - 1.0 ? tx : G.nx - 1.0) : 0.0;
  ty = ty >= 0.0 ? (ty <= G.ny - 1.0 ? ty : G.ny - 1.0) : 0.0;
  const int b = static_cast<int>(floor(ty)) * G.nx + static_cast<int>(floor(tx));
  int found = -1;
  l0 = l1 = l2 = __builtin_nan("");
  for (int k = G.start[b], e = G.start[b + 1]; k < e; ++k) {
    const int c = G.cells[k];
    if (c < 0 || c >= nc) continue;
    double m0, m1, m2;
    if (point_in_cell(xy, nc, c, px, py, m0, m1, m2)) {
      found = c;
      l0 = m0;
      l1 = m1;
      l2 = m2;
      break;
    }
  }
  return found;
}

// one point per lane
__global__ __launch_bounds__(kBlock) void locate_points_kernel(
    int nc, const double* __restrict__ xy, const flow_point_grid G, int n,
    const double* __restrict__ pts, int* __restrict__ cell,
    double* __restrict__ bary) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double px = pts[i], py = pts[static_cast<size_t>(n) + i];
  double l0, l1, l2;
  cell[i] = locate_point(xy, nc, G, px, py, l0, l1, l2);
  bary[i] = l0;
  bary[static_cast<size_t>(n) + i] = l1;
  bary[2 * static_cast<size_t>(n) + i] = l2;
}

// ---------------------------------------------------------------------------
// Tracer particles (flow_amd/fem/tracers.py, flow_advect_points): one particle
// per lane; its position, cell and barycentric coordinates stay in registers
// over all `steps` substeps of an explicit Runge-Kutta scheme (SCHEME 1: Euler,
// 2: midpoint, 4: classical RK4).  Every stage point is located with
// locate_point -- the exact lowest-index scan, so a stage's velocity is a
// function of the point alone and steps = k equals k calls of steps = 1 bit
// for bit -- and the P1 / P2 velocity is evaluated there from the cell's dofs.
// NEXT: the velocity at fraction theta of the call's time steps * dt is
// (1 - theta) u + theta u_next.  A substep one of whose stage points, or whose
// end point, lies in no cell loses the particle: it keeps the position it had
// at the start of that substep, its cell becomes -1 and the lane stops
// loading.  The end point of an accepted substep is the first stage point of
// the next one, so a substep of s stages costs s locations.  No atomics, no
// LDS, no reductions; the only divergence is the bucket scan and the loss.
// ---------------------------------------------------------------------------
template <int DEG, bool NEXT>
__device__ __forceinline__ void tracer_velocity(
    int nc, int c, double l0, double l1, double l2,
    const int* __restrict__ cell_dofs, int ndof, const double* __restrict__ u,
    const double* __restrict__ u_next, double theta, double& vx, double& vy) {
  constexpr int NL = Elem<DEG>::NL;
  const double L[3] = {l0, l1, l2};
  int d[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) d[j] = cell_dofs[j * nc + c];
  double U[2][NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    U[0][j] = u[d[j]];
    U[1][j] = u[static_cast<size_t>(ndof) + d[j]];
  }
  vx = eval_at<DEG>(U[0], L);
  vy = eval_at<DEG>(U[1], L);
  if constexpr (NEXT) {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      U[0][j] = u_next[d[j]];
      U[1][j] = u_next[static_cast<size_t>(ndof) + d[j]];
    }
    vx = (1.0 - theta) * vx + theta * eval_at<DEG>(U[0], L);
    vy = (1.0 - theta) * vy + theta * eval_at<DEG>(U[1], L);
  }
}

template <int DEG, int SCHEME, bool NEXT>
__global__ __launch_bounds__(kBlock) void advect_points_kernel(
    int nc, const double* __restrict__ xy, const flow_point_grid G,
    const int* __restrict__ cell_dofs, int ndof, const double* __restrict__ u,
    const double* __restrict__ u_next, int n, double* __restrict__ pts,
    int* __restrict__ cell, double* __restrict__ bary, double dt, int steps) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int c = cell[i];
  if (c < 0 || c >= nc) return;          // lost: left alone
  double px = pts[i], py = pts[static_cast<size_t>(n) + i];
  double l0 = bary[i], l1 = bary[static_cast<size_t>(n) + i],
         l2 = bary[2 * static_cast<size_t>(n) + i];
  const double inv_steps = 1.0 / steps;
  for (int s = 0; s < steps; ++s) {
    // (cs, m) the cell and the barycentrics of a stage point, (ex, ey) the
    // end point
    double k1x, k1y, ex = px, ey = py;
    tracer_velocity<DEG, NEXT>(nc, c, l0, l1, l2, cell_dofs, ndof, u, u_next,
                               s * inv_steps, k1x, k1y);
    bool ok = true;
    if constexpr (SCHEME == 1) {
      ex = px + dt * k1x;
      ey = py + dt * k1y;
    } else {
      const double th = (s + 0.5) * inv_steps;
      double m0, m1, m2, k2x, k2y;
      int cs = locate_point(xy, nc, G, px + (0.5 * dt) * k1x, py + (0.5 * dt) * k1y,
                            m0, m1, m2);
      ok = cs >= 0;
      if (ok) {
        tracer_velocity<DEG, NEXT>(nc, cs, m0, m1, m2, cell_dofs, ndof, u, u_next,
                                   th, k2x, k2y);
        if constexpr (SCHEME == 2) {
          ex = px + dt * k2x;
          ey = py + dt * k2y;
        } else {
          double k3x, k3y, k4x, k4y;
          cs = locate_point(xy, nc, G, px + (0.5 * dt) * k2x,
                            py + (0.5 * dt) * k2y, m0, m1, m2);
          ok = cs >= 0;
          if (ok) {
            tracer_velocity<DEG, NEXT>(nc, cs, m0, m1, m2, cell_dofs, ndof, u,
                                       u_next, th, k3x, k3y);
            cs = locate_point(xy, nc, G, px + dt * k3x, py + dt * k3y, m0, m1, m2);
            ok = cs >= 0;
          }
          if (ok) {
            tracer_velocity<DEG, NEXT>(nc, cs, m0, m1, m2, cell_dofs, ndof, u,
                                       u_next, (s + 1) * inv_steps, k4x, k4y);
            ex = px + (dt / 6.0) * (k1x + 2.0 * k2x + 2.0 * k3x + k4x);
            ey = py + (dt / 6.0) * (k1y + 2.0 * k2y + 2.0 * k3y + k4y);
          }
        }
      }
    }
    int ce = -1;
    double e0, e1, e2;
    if (ok) ce = locate_point(xy, nc, G, ex, ey, e0, e1, e2);
    if (ce < 0) {
      // lost: the position of the start of this substep stays
      c = -1;
      l0 = l1 = l2 = __builtin_nan("");
      break;
    }
    px = ex;
    py = ey;
    c = ce;
    l0 = e0;
    l1 = e1;
    l2 = e2;
  }
  pts[i] = px;
  pts[static_cast<size_t>(n) + i] = py;
  cell[i] = c;
  bary[i] = l0;
  bary[static_cast<size_t>(n) + i] = l1;
  bary[2 * static_cast<size_t>(n) + i] = l2;
}

// one located point per lane: the program at its barycentric coordinates,
// out[o][i]; NaN for a point in no cell
template <int NF, bool EXT>
__global__ __launch_bounds__(kBlock) void form_points_kernel(
    int nc, const double* __restrict__ xy, const flow_form F, int n,
    const int* __restrict__ cell, const double* __restrict__ bary,
    double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = cell[i];
  double out0 = __builtin_nan(""), out1 = out0;
  if (c >= 0 && c < nc) {
    FormCell<NF> C;
    load_form_cell<NF>(F, nc, xy, c, C);
    const double L[3] = {bary[i], bary[static_cast<size_t>(n) + i],
                         bary[2 * static_cast<size_t>(n) + i]};
    out0 = 0.0;
    out1 = 0.0;
    form_point<NF, false, EXT>(F, C.U, C.X, C.Y, C.g, L, 0, nc, c, 0.0, 0.0, out0, out1);
  }
  out[i] = out0;
  if (F.nout == 2) out[static_cast<size_t>(n) + i] = out1;
}

// ---------------------------------------------------------------------------
// Forms of test and trial functions (forms.py, extract_arguments): the host
// rewrites a rank-2 integrand as sum_(b,a) c_ba D_a u D_b v and a rank-1
// integrand as sum_b c_b D_b v (D_0 value, D_1 d/dx, D_2 d/dy), and compiles
// the argument-free coefficients c into ONE program whose output slot is fixed
// by the term: 3 b + a (rank 2), b (rank 1).  `live` holds one bit per slot
// the program writes; it is a kernel argument, so a term that is absent costs
// a wave-uniform branch and nothing else.
// ---------------------------------------------------------------------------
// D_a of basis function t (a is a compile-time value in the unrolled callers)
template <int NL>
__device__ __forceinline__ double arg_basis(int a, const double (&phi)[NL],
                                            const double (&gphi)[NL][2], int t) {
  return a == 0 ? phi[t] : gphi[t][a == 2 ? 1 : 0];
}

// The rank-2 accumulation of one point, shared by form_matrix_kernel and the
// facet kernel (form_newton_kernel restates it; the bit-for-bit tests check
// that copy).  m is the mask of live slots, w the point's weight, slots the
// program's outputs; `base` is the position of the table in both.
//
// t_j = sum_a w c_ba D_a phi_j for one test derivative b, whose three slots
// (a = 0, 1, 2) start at `first`
template <int NL, int NS>
__device__ __forceinline__ void trial_sums(int m, int first, double w,
                                           const double (&slots)[NS],
                                           const double (&phi)[NL],
                                           const double (&gphi)[NL][2], double (&t)[NL]) {
#pragma unroll
  for (int j = 0; j < NL; ++j) t[j] = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (((m >> (first + a)) & 1) == 0) continue;
    const double s = w * slots[first + a];
#pragma unroll
    for (int j = 0; j < NL; ++j) t[j] += s * arg_basis<NL>(a, phi, gphi, j);
  }
}

// rank 2: per test derivative b, t_j first, then Ke[i][j] += D_b phi_i t_j
template <int NL, int NS>
__device__ __forceinline__ void add_matrix_terms(int m, int base, double w,
                                                 const double (&slots)[NS],
                                                 const double (&phi)[NL],
                                                 const double (&gphi)[NL][2],
                                                 double (&Ke)[NL][NL]) {
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    if (((m >> (base + 3 * b)) & 7) == 0) continue;
    double t[NL];
    trial_sums<NL>(m, base + 3 * b, w, slots, phi, gphi, t);
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const double di = arg_basis<NL>(b, phi, gphi, i);
#pragma unroll
      for (int j = 0; j < NL; ++j) Ke[i][j] += di * t[j];
    }
  }
}

// D_b of the basis function `own`, which the lane knows at run time only
// (selects: a run-time index would put the tables in scratch memory)
template <int NL>
__device__ __forceinline__ double own_basis(int b, const double (&phi)[NL],
                                            const double (&gphi)[NL][2], int own) {
  double d = 0.0;
#pragma unroll
  for (int t = 0; t < NL; ++t) d = t == own ? arg_basis<NL>(b, phi, gphi, t) : d;
  return d;
}

// Ke[i][j] = sum_q w_q |det J| sum_ba c_ba(x_q) D_a phi_j D_b phi_i, to
// scratch[(i*NL + j)*nc + c] (the layout of scalar_matrix_kernel: the gather
// over cptr / csrc sums it into a value plane).  All NL*NL entries are held
// in one pass over the rule (measured faster than a row or three
// at a time with the program re-run per pass).  Per point and test derivative
// b, t_j = sum_a w c_ba D_a phi_j first, then Ke[i][j] += D_b phi_i t_j.
// (form_cells_matrix_kernel below restates this kernel over a cell list and
// must give its bits: an edit here is an edit there)
template <int NF, int DEG, bool EXT>
__global__ __launch_bounds__(kBlock) void form_matrix_kernel(
    int nc, const double* __restrict__ xy, const flow_form F, int live,
    double* __restrict__ scratch) {
  constexpr int NL = Elem<DEG>::NL;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  // (the lane's own address: the base pointer need not stay in scalar
  // registers across the interpreter loop, which is short of them)
  double* const dst = scratch + c;
  FormCell<NF> C;
  load_form_cell<NF>(F, nc, xy, c, C);
  double Ke[NL][NL];
#pragma unroll
  for (int i = 0; i < NL; ++i)
#pragma unroll
    for (int j = 0; j < NL; ++j) Ke[i][j] = 0.0;
  for (int q = 0; q < F.nq; ++q) {
    const double xi = F.rule[3 * q], eta = F.rule[3 * q + 1];
    const double w = F.rule[3 * q + 2] * C.g.adet;
    const double L[3] = {1.0 - xi - eta, xi, eta};
    FormSlots<FLOW_FORM_SLOTS> out;
#pragma unroll
    for (int k = 0; k < FLOW_FORM_SLOTS; ++k) out.v[k] = 0.0;
    form_point_n<NF, false, EXT>(F, C.U, C.X, C.Y, C.g, L, q, nc, c, 0.0, 0.0, out);
    double phi[NL], dphi[NL][3], gphi[NL][2];
    basis<DEG>(L, phi, dphi);
    phys_grad<NL>(C.g, dphi, gphi);
    // (the mask through an empty asm: otherwise the twelve tests of the
    // accumulation are hoisted out of the loop and their results held in
    // scalar registers across the interpreter, which then spills two of its
    // own)
    int m = live;
    asm volatile("" : "+s"(m));
    add_matrix_terms<NL>(m, 0, w, out.v, phi, gphi, Ke);
  }
#pragma unroll
  for (int i = 0; i < NL; ++i)
#pragma unroll
    for (int j = 0; j < NL; ++j)
      dst[static_cast<size_t>(i * NL + j) * nc] = Ke[i][j];
}

// be[i] = sum_q w_q |det J| sum_b c_b(x_q) D_b phi_i, to scratch[i*nc + c]
// (the gather over vptr / vsrc sums it into the vector; form_cells_vector_kernel
// below restates this kernel over a cell list and must give its bits: an edit
// here is an edit there)
template <int NF, int DEG, bool EXT>
__global__ __launch_bounds__(kBlock) void form_vector_kernel(
    int nc, const double* __restrict__ xy, const flow_form F, int live,
    double* __restrict__ scratch) {
  constexpr int NL = Elem<DEG>::NL;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  // (this kernel keeps its own statement of the cell prologue and of its
  // accumulation: built from load_form_cell and a routine for the loop, two
  // of its 28 instances take more registers)
  const Geom g = load_geom(xy, nc, c);
  const double X[3] = {xy[0 * nc + c], xy[1 * nc + c], xy[2 * nc + c]};
  const double Y[3] = {xy[3 * nc + c], xy[4 * nc + c], xy[5 * nc + c]};
  double U[NF > 0 ? NF : 1][6];
  load_form_fields<NF>(F, nc, c, U);
  double be[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) be[i] = 0.0;
  for (int q = 0; q < F.nq; ++q) {
    const double xi = F.rule[3 * q], eta = F.rule[3 * q + 1];
    const double w = F.rule[3 * q + 2] * g.adet;
    const double L[3] = {1.0 - xi - eta, xi, eta};
    FormSlots<3> out = {{0.0, 0.0, 0.0}};
    form_point_n<NF, false, EXT>(F, U, X, Y, g, L, q, nc, c, 0.0, 0.0, out);
    double phi[NL], dphi[NL][3], gphi[NL][2];
    basis<DEG>(L, phi, dphi);
    phys_grad<NL>(g, dphi, gphi);
    // (EXT: the mask through an empty asm, as in form_matrix_kernel -- the
    // larger interpreter has no scalar registers left for the hoisted tests)
    int m = live;
    if constexpr (EXT) asm volatile("" : "+s"(m));
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      if (((m >> b) & 1) == 0) continue;
      const double s = w * out.v[b];
#pragma unroll
      for (int i = 0; i < NL; ++i) be[i] += s * arg_basis<NL>(b, phi, gphi, i);
    }
  }
#pragma unroll
  for (int i = 0; i < NL; ++i) scratch[static_cast<size_t>(i) * nc + c] = be[i];
}

// Jacobian and residual of a Newton iteration in one pass (forms.py,
// newton_program): ONE program writes the 9 slots of the Jacobian's table and,
// at 9 + b, the 3 of the residual's; geometry, field values, basis tables and
// the subtrees the two tables share are loaded / computed once per point.  Ke
// and be are accumulated with the arithmetic of form_matrix_kernel
// (add_matrix_terms) and form_vector_kernel, in their order; Ke goes to
// scratch[(i*NL + j)*nc + c], be behind it to scratch[(NL*NL + i)*nc + c].
// live: bits 0..8 the Jacobian's slots, 9..11 the residual's.
template <int NF, int DEG, bool EXT>
__global__ __launch_bounds__(kBlock) void form_newton_kernel(
    int nc, const double* __restrict__ xy, const flow_form F, int live,
    double* __restrict__ scratch) {
  constexpr int NL = Elem<DEG>::NL;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  double* const dst = scratch + c;
  // (this kernel keeps its own statement of the cell prologue and of the two
  // accumulations: built from load_form_cell and add_matrix_terms its P2
  // instances measured 1.4 % slower in the block Newton pass)
  const Geom g = load_geom(xy, nc, c);
  const double X[3] = {xy[0 * nc + c], xy[1 * nc + c], xy[2 * nc + c]};
  const double Y[3] = {xy[3 * nc + c], xy[4 * nc + c], xy[5 * nc + c]};
  double U[NF > 0 ? NF : 1][6];
  load_form_fields<NF>(F, nc, c, U);
  double Ke[NL][NL], be[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    be[i] = 0.0;
#pragma unroll
    for (int j = 0; j < NL; ++j) Ke[i][j] = 0.0;
  }
  for (int q = 0; q < F.nq; ++q) {
    const double xi = F.rule[3 * q], eta = F.rule[3 * q + 1];
    const double w = F.rule[3 * q + 2] * g.adet;
    const double L[3] = {1.0 - xi - eta, xi, eta};
    FormSlots<FLOW_FORM_NEWTON_SLOTS> out;
#pragma unroll
    for (int k = 0; k < FLOW_FORM_NEWTON_SLOTS; ++k) out.v[k] = 0.0;
    form_point_n<NF, false, EXT>(F, U, X, Y, g, L, q, nc, c, 0.0, 0.0, out);
    double phi[NL], dphi[NL][3], gphi[NL][2];
    basis<DEG>(L, phi, dphi);
    phys_grad<NL>(g, dphi, gphi);
    // (the mask through an empty asm, as in form_matrix_kernel)
    int m = live;
    asm volatile("" : "+s"(m));
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      if (((m >> (3 * b)) & 7) == 0) continue;
      double t[NL];
#pragma unroll
      for (int j = 0; j < NL; ++j) t[j] = 0.0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (((m >> (3 * b + a)) & 1) == 0) continue;
        const double s = w * out.v[3 * b + a];
#pragma unroll
        for (int j = 0; j < NL; ++j) t[j] += s * arg_basis<NL>(a, phi, gphi, j);
      }
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const double di = arg_basis<NL>(b, phi, gphi, i);
#pragma unroll
        for (int j = 0; j < NL; ++j) Ke[i][j] += di * t[j];
      }
    }
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      if (((m >> (FLOW_FORM_SLOTS + b)) & 1) == 0) continue;
      const double s = w * out.v[FLOW_FORM_SLOTS + b];
#pragma unroll
      for (int i = 0; i < NL; ++i) be[i] += s * arg_basis<NL>(b, phi, gphi, i);
    }
  }
#pragma unroll
  for (int i = 0; i < NL; ++i)
#pragma unroll
    for (int j = 0; j < NL; ++j)
      dst[static_cast<size_t>(i * NL + j) * nc] = Ke[i][j];
#pragma unroll
  for (int i = 0; i < NL; ++i)
    dst[static_cast<size_t>(NL * NL + i) * nc] = be[i];
}

// ---------------------------------------------------------------------------
// Forms of arguments over exterior facets (Neumann, Robin and Nitsche terms:
// g*v*ds, h*u*v*ds, dot(grad(u), n)*v*ds).  A boundary holds O(sqrt(N))
// facets, so a facet is shared by NL lanes: lane (i, k) -- k the position in
// the facet list, fastest -- holds row i of the element matrix of facet k's
// owning cell (RANK 2: NL doubles) or entry i of its element vector (RANK 1:
// one).  ALL NL basis functions of the cell take part: the gradient of the
// off-edge one does not vanish on the edge.  Geometry, normal, edge length
// and the rows of the rule are those of form_facet; per point the arithmetic
// is that of form_matrix_kernel / form_vector_kernel with w = rule weight x
// edge length: t_j = sum_a w c_ba D_a phi_j, then Ke[i][j] += D_b phi_i t_j.
// Entries go to scratch[(i*NL + j)*nfacets + k] (RANK 2) or
// scratch[i*nfacets + k] (RANK 1); facet_gather_kernel sums them.  A facet
// outside the mesh gives NaN, not a stray read.
// ---------------------------------------------------------------------------
template <int NF, int DEG, bool EXT, int RANK>
__global__ __launch_bounds__(kBlock) void form_facet_arguments_kernel(
    int nc, int nfacets, const int* __restrict__ fcell,
    const int* __restrict__ flocal, const double* __restrict__ xy,
    const flow_form F, int live, double* __restrict__ scratch) {
  constexpr int NL = Elem<DEG>::NL;
  constexpr int NR = RANK == 2 ? NL : 1;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nfacets * NL) return;
  const int i = idx / nfacets, k = idx - i * nfacets;
  double* const dst = scratch + static_cast<size_t>(i) * NR * nfacets + k;
  const int c = fcell[k], lf = flocal[k];
  if (c < 0 || c >= nc || lf < 0 || lf > 2) {
#pragma unroll
    for (int j = 0; j < NR; ++j)
      dst[static_cast<size_t>(j) * nfacets] = __builtin_nan("");
    return;
  }
  FormCell<NF> C;
  load_form_cell<NF>(F, nc, xy, c, C);
  const FacetFrame f = facet_frame(C.g, lf);
  double acc[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) acc[j] = 0.0;
  for (int q = 0; q < F.nq; ++q) {
    const int row = lf * F.nq + q;
    const double xi = F.rule[3 * row], eta = F.rule[3 * row + 1];
    const double w = F.rule[3 * row + 2] * f.len;
    const double L[3] = {1.0 - xi - eta, xi, eta};
    FormSlots<RANK == 2 ? FLOW_FORM_SLOTS : 3> out;
#pragma unroll
    for (int s = 0; s < (RANK == 2 ? FLOW_FORM_SLOTS : 3); ++s) out.v[s] = 0.0;
    form_point_n<NF, true, EXT>(F, C.U, C.X, C.Y, C.g, L, row, nc, c, f.n0, f.n1, out);
    double phi[NL], dphi[NL][3], gphi[NL][2];
    basis<DEG>(L, phi, dphi);
    phys_grad<NL>(C.g, dphi, gphi);
    // (the mask through an empty asm, as in form_matrix_kernel)
    int m = live;
    asm volatile("" : "+s"(m));
    if constexpr (RANK == 2) {
      // row i of add_matrix_terms
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        if (((m >> (3 * b)) & 7) == 0) continue;
        const double di = own_basis<NL>(b, phi, gphi, i);
        double t[NL];
        trial_sums<NL>(m, 3 * b, w, out.v, phi, gphi, t);
#pragma unroll
        for (int j = 0; j < NL; ++j) acc[j] += di * t[j];
      }
    } else {
      // entry i of the loop of form_vector_kernel (stated here: through a
      // routine two of the 28 rank-1 instances change their register counts,
      // DESIGN.md)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        if (((m >> b) & 1) == 0) continue;
        const double di = own_basis<NL>(b, phi, gphi, i);
        acc[0] += (w * out.v[b]) * di;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NR; ++j) dst[static_cast<size_t>(j) * nfacets] = acc[j];
}

// The gather over the facet contribution map (ops.facet_map): one lane per
// target adds scratch[src[e]], e in [ptr[t], ptr[t+1]), in that order and
// writes out[targets[t]]; the rest of `out` is not touched.  No atomics: two
// calls give the same bits.  A target outside `out` is skipped; a row of ptr or
// an entry of src outside the scratch gives NaN, not a stray read.
__global__ __launch_bounds__(kBlock) void facet_gather_kernel(
    int ntargets, const int* __restrict__ targets, const int* __restrict__ ptr,
    const int* __restrict__ src, int nsrc, const double* __restrict__ scratch,
    int nout, double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntargets) return;
  const int tg = targets[t];
  if (tg < 0 || tg >= nout) return;
  const int b = ptr[t], e = ptr[t + 1];
  double s = 0.0;
  if (b < 0 || e > nsrc || b > e) {
    s = __builtin_nan("");
  } else {
    for (int q = b; q < e; ++q) {
      const int x = src[q];
      s += (x >= 0 && x < nsrc) ? scratch[x] : __builtin_nan("");
    }
  }
  out[tg] = s;
}

// ---------------------------------------------------------------------------
// Cell subdomains (assemble(f*dx(k)), flow_form_cells_*): the cell-list forms
// of form_cell_kernel (TD = 0), form_matrix_kernel and form_vector_kernel.
// Lane k of nsel takes c = cells[k], runs the arithmetic of the whole-mesh
// kernel on cell c -- the same rule order, add_matrix_terms, the same handling
// of the live mask -- and stores with stride nsel at position k; a list that
// holds every cell in ascending order gives the bits of the whole-mesh kernel.
// They are kernels of their own, not a parameter of the whole-mesh ones:
// those are short of scalar registers (see the comments there), and a list
// pointer and a count more would change their instances.  A list
// entry outside [0, nc) gives NaN, not a stray read.
// ---------------------------------------------------------------------------
// BY_CELL = false: out[k] = the integral over cell cells[k] (the functional's
// stage 1); true: out[cells[k]] (flow_form_cells_values: the caller zeroed
// out, an entry outside the mesh is skipped)
template <int NF, bool EXT, bool BY_CELL>
__global__ __launch_bounds__(kBlock) void form_cells_kernel(
    int nc, int nsel, const int* __restrict__ cells, const double* __restrict__ xy,
    const flow_form F, double* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nsel) return;
  const int c = cells[k];
  if (c < 0 || c >= nc) {
    if constexpr (!BY_CELL) out[k] = __builtin_nan("");
    return;
  }
  double acc[2][6];
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[o][i] = 0.0;
  out[BY_CELL ? c : k] = form_cell<NF, 0, EXT>(F, nc, xy, c, acc);
}

// Ke of cell cells[k] to scratch[(i*NL + j)*nsel + k]: form_matrix_kernel
// over a list
template <int NF, int DEG, bool EXT>
__global__ __launch_bounds__(kBlock) void form_cells_matrix_kernel(
    int nc, int nsel, const int* __restrict__ cells, const double* __restrict__ xy,
    const flow_form F, int live, double* __restrict__ scratch) {
  constexpr int NL = Elem<DEG>::NL;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nsel) return;
  double* const dst = scratch + k;
  const int c = cells[k];
  if (c < 0 || c >= nc) {
#pragma unroll
    for (int ij = 0; ij < NL * NL; ++ij)
      dst[static_cast<size_t>(ij) * nsel] = __builtin_nan("");
    return;
  }
  FormCell<NF> C;
  load_form_cell<NF>(F, nc, xy, c, C);
  double Ke[NL][NL];
#pragma unroll
  for (int i = 0; i < NL; ++i)
#pragma unroll
    for (int j = 0; j < NL; ++j) Ke[i][j] = 0.0;
  for (int q = 0; q < F.nq; ++q) {
    const double xi = F.rule[3 * q], eta = F.rule[3 * q + 1];
    const double w = F.rule[3 * q + 2] * C.g.adet;
    const double L[3] = {1.0 - xi - eta, xi, eta};
    FormSlots<FLOW_FORM_SLOTS> out;
#pragma unroll
    for (int s = 0; s < FLOW_FORM_SLOTS; ++s) out.v[s] = 0.0;
    form_point_n<NF, false, EXT>(F, C.U, C.X, C.Y, C.g, L, q, nc, c, 0.0, 0.0, out);
    double phi[NL], dphi[NL][3], gphi[NL][2];
    basis<DEG>(L, phi, dphi);
    phys_grad<NL>(C.g, dphi, gphi);
    // (the mask through an empty asm, as in form_matrix_kernel)
    int m = live;
    asm volatile("" : "+s"(m));
    add_matrix_terms<NL>(m, 0, w, out.v, phi, gphi, Ke);
  }
#pragma unroll
  for (int i = 0; i < NL; ++i)
#pragma unroll
    for (int j = 0; j < NL; ++j)
      dst[static_cast<size_t>(i * NL + j) * nsel] = Ke[i][j];
}

// be of cell cells[k] to scratch[i*nsel + k]: form_vector_kernel over a list
template <int NF, int DEG, bool EXT>
__global__ __launch_bounds__(kBlock) void form_cells_vector_kernel(
    int nc, int nsel, const int* __restrict__ cells, const double* __restrict__ xy,
    const flow_form F, int live, double* __restrict__ scratch) {
  constexpr int NL = Elem<DEG>::NL;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nsel) return;
  const int c = cells[k];
  if (c < 0 || c >= nc) {
#pragma unroll
    for (int i = 0; i < NL; ++i)
      scratch[static_cast<size_t>(i) * nsel + k] = __builtin_nan("");
    return;
  }
  const Geom g = load_geom(xy, nc, c);
  const double X[3] = {xy[0 * nc + c], xy[1 * nc + c], xy[2 * nc + c]};
  const double Y[3] = {xy[3 * nc + c], xy[4 * nc + c], xy[5 * nc + c]};
  double U[NF > 0 ? NF : 1][6];
  load_form_fields<NF>(F, nc, c, U);
  double be[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) be[i] = 0.0;
  for (int q = 0; q < F.nq; ++q) {
    const double xi = F.rule[3 * q], eta = F.rule[3 * q + 1];
    const double w = F.rule[3 * q + 2] * g.adet;
    const double L[3] = {1.0 - xi - eta, xi, eta};
    FormSlots<3> out = {{0.0, 0.0, 0.0}};
    form_point_n<NF, false, EXT>(F, U, X, Y, g, L, q, nc, c, 0.0, 0.0, out);
    double phi[NL], dphi[NL][3], gphi[NL][2];
    basis<DEG>(L, phi, dphi);
    phys_grad<NL>(g, dphi, gphi);
    // (EXT: the mask through an empty asm, as in form_vector_kernel)
    int m = live;
    if constexpr (EXT) asm volatile("" : "+s"(m));
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      if (((m >> b) & 1) == 0) continue;
      const double s = w * out.v[b];
#pragma unroll
      for (int i = 0; i < NL; ++i) be[i] += s * arg_basis<NL>(b, phi, gphi, i);
    }
  }
#pragma unroll
  for (int i = 0; i < NL; ++i) scratch[static_cast<size_t>(i) * nsel + k] = be[i];
}

// rows: the rule holds rows * nq points (1: cells; 3: the three local
// facets); facet: NORMAL is legal; points: the program runs at located
// points -- no rule, no Expression lattices (they are tabulated at the
// rule's rows), no normal; slots = 0: one or two outputs, each written; 9 | 3:
// the coefficient table of a rank-2 | rank-1 form, 12: the two tables of
// flow_form_newton behind one another -- nout == slots, *live = one bit per
// slot the program writes (at least one, none twice; 12: at least one of the
// first 9 and one of the last 3)
static int check_form(const flow_form* F, int rows = 1, bool facet = false,
                      bool points = false, int slots = 0, int* live = nullptr,
                      int* minus_slots = nullptr) {
  // minus_slots != nullptr: the program of an interior facet (with facet =
  // true).  There, and only there, FIELD / NORMAL / CELL may carry their side
  // bit and FACET_LEN exists; EXPR does not (its tables are indexed by the
  // rule's row of one cell).  *minus_slots = one bit per field slot that is
  // read on the '-' cell; a slot is read on one side only
  const bool interior = minus_slots != nullptr;
  int plus = 0, minus = 0;
  FLOW_REQUIRE(F, "form");
  FLOW_REQUIRE(F->nprog >= 1 && F->nprog <= FLOW_FORM_MAX_PROGRAM,
               "form program length");
  FLOW_REQUIRE(F->nconst >= 0 && F->nconst <= FLOW_FORM_MAX_CONSTANTS,
               "form constants");
  FLOW_REQUIRE(F->nfield >= 0 && F->nfield <= FLOW_FORM_MAX_FIELDS, "form fields");
  FLOW_REQUIRE(F->nexpr >= 0 && F->nexpr <= FLOW_FORM_MAX_EXPRESSIONS,
               "form expressions");
  FLOW_REQUIRE(slots == 0 ? (F->nout == 1 || F->nout == 2) : (F->nout == slots && live),
               "form outputs");
  FLOW_REQUIRE(points || (F->nq >= 1 && rows * F->nq <= FLOW_FORM_MAX_POINTS && F->rule),
               "form quadrature rule");
  FLOW_REQUIRE(!points || F->nexpr == 0,
               "form expression (Expression leaves cannot be evaluated at points)");
  for (int k = 0; k < F->nfield; ++k) {
    FLOW_REQUIRE(F->field[k], "form field pointer");
    FLOW_REQUIRE(F->field_deg[k] == 1 || F->field_deg[k] == 2, "form field degree");
    FLOW_REQUIRE(F->cell_dofs[F->field_deg[k] - 1], "form field cell_dofs");
  }
  for (int k = 0; k < F->nexpr; ++k) {
    FLOW_REQUIRE(F->expr[k] && F->expr_nl[k] >= 1 && F->expr_nl[k] <= 21,
                 "form expression lattice");
    FLOW_REQUIRE(F->tables && F->expr_table[k] >= 0 &&
                     F->expr_table[k] + rows * F->nq * F->expr_nl[k] <= F->ntables,
                 "form expression table");
  }
  // every instruction: registers, operand indices and outputs in range (the
  // kernel indexes kernel-argument arrays with them)
  int wrote = 0;
  for (int pc = 0; pc < F->nprog; ++pc) {
    const int op = F->prog[4 * pc], dst = F->prog[4 * pc + 1];
    const int a = F->prog[4 * pc + 2], b = F->prog[4 * pc + 3];
    FLOW_REQUIRE((op >= FLOW_FORM_OP_CONST && op <= FLOW_FORM_OP_OUT) ||
                     (facet && op == FLOW_FORM_OP_NORMAL) ||
                     (op >= FLOW_FORM_OP_LT && op <= FLOW_FORM_OP_CELL) ||
                     (interior && op == FLOW_FORM_OP_FACET_LEN),
                 facet ? "form opcode (FACET_LEN: interior facets only)"
                       : "form opcode (NORMAL: facet integrals only)");
    FLOW_REQUIRE(!points || op != FLOW_FORM_OP_EXPR,
                 "form opcode (EXPR: not at points)");
    FLOW_REQUIRE(!interior || op != FLOW_FORM_OP_EXPR,
                 "form opcode (EXPR: not on interior facets)");
    // the side bits: legal on interior facets, out of range anywhere else
    const int side_f = interior ? FLOW_FORM_SIDE_FIELD : 0;
    const int side_n = interior ? FLOW_FORM_SIDE_NORMAL : 0;
    const int side_c = interior ? FLOW_FORM_SIDE_CELL : 0;
    const bool reg_a = (op >= FLOW_FORM_OP_MOV && op <= FLOW_FORM_OP_OUT) ||
                       (op >= FLOW_FORM_OP_LT && op <= FLOW_FORM_OP_TANH);
    const bool reg_b = (op >= FLOW_FORM_OP_ADD && op <= FLOW_FORM_OP_POW) ||
                       (op >= FLOW_FORM_OP_LT && op <= FLOW_FORM_OP_MAX);
    FLOW_REQUIRE(dst >= 0 && dst < FLOW_FORM_REGISTERS, "form register");
    FLOW_REQUIRE(!reg_a || (a >= 0 && a < FLOW_FORM_REGISTERS), "form register");
    FLOW_REQUIRE(!reg_b || (b >= 0 && b < FLOW_FORM_REGISTERS), "form register");
    switch (op) {
      case FLOW_FORM_OP_CONST:
        FLOW_REQUIRE(a >= 0 && a < F->nconst, "form constant index");
        break;
      case FLOW_FORM_OP_COORD:
        FLOW_REQUIRE(a == 0 || a == 1, "form coordinate");
        break;
      case FLOW_FORM_OP_FIELD:
        FLOW_REQUIRE(a >= 0 && a < F->nfield && b >= 0 && (b & ~side_f) <= 2,
                     "form field operand (a side bit: interior facets only)");
        if (interior) {
          if (b & side_f) minus |= 1 << a;
          else plus |= 1 << a;
        }
        break;
      case FLOW_FORM_OP_EXPR:
        FLOW_REQUIRE(a >= 0 && a < F->nexpr, "form expression index");
        break;
      case FLOW_FORM_OP_NORMAL:
        FLOW_REQUIRE(a >= 0 && (a & ~side_n) <= 1,
                     "form normal component (a side bit: interior facets only)");
        break;
      case FLOW_FORM_OP_CELL:
        FLOW_REQUIRE(a >= 0 && (a & ~side_c) <= 2,
                     "form cell quantity (a side bit: interior facets only)");
        break;
      case FLOW_FORM_OP_OUT:
        FLOW_REQUIRE(b >= 0 && b < F->nout, "form output");
        FLOW_REQUIRE(slots == 0 || !((wrote >> b) & 1), "form output slot written twice");
        wrote |= 1 << b;
        break;
      default: break;
    }
  }
  if (slots == 0)
    FLOW_REQUIRE(wrote == (1 << F->nout) - 1, "form writes every output");
  else
    FLOW_REQUIRE(wrote != 0, "form writes no coefficient slot");
  if (slots == FLOW_FORM_NEWTON_SLOTS)
    FLOW_REQUIRE((wrote & ((1 << FLOW_FORM_SLOTS) - 1)) != 0 && (wrote >> FLOW_FORM_SLOTS) != 0,
                 "form writes no Jacobian slot or no residual slot");
  if (live) *live = wrote;
  if (interior) {
    FLOW_REQUIRE((plus & minus) == 0, "form field slot read on both sides");
    *minus_slots = minus;
  }
  return FLOW_OK;
}

// whether the program holds an extended opcode: it then runs on the EXT
// instance of its kernel
static bool form_is_extended(const flow_form* F) {
  for (int pc = 0; pc < F->nprog; ++pc)
    if (F->prog[4 * pc] >= FLOW_FORM_OP_LT && F->prog[4 * pc] <= FLOW_FORM_OP_CELL)
      return true;
  return false;
}

static int check_form_mesh(const flow_mesh* mesh) {
  FLOW_REQUIRE(mesh && mesh->nc > 0 && mesh->xy, "mesh");
  FLOW_REQUIRE(mesh->c1 == 0 ||
                   (0 <= mesh->c0 && mesh->c0 < mesh->c1 && mesh->c1 <= mesh->nc),
               "mesh cell range");
  return FLOW_OK;
}

// what every entry point of a form of arguments asks of its mesh and space:
// the whole mesh, a space of degree 1 or 2 with the gather maps of the
// element matrices (need_matrix) and / or vectors (need_vector)
static int check_argument_space(const flow_mesh* mesh, const flow_space* V,
                                bool need_matrix, bool need_vector) {
  const int rc = check_form_mesh(mesh);
  if (rc) return rc;
  FLOW_REQUIRE(mesh->c1 == 0, "forms of arguments on strips");
  FLOW_REQUIRE(V && (V->deg == 1 || V->deg == 2) && V->n > 0 &&
                   (!need_matrix || (V->nnz > 0 && V->cptr && V->csrc)) &&
                   (!need_vector || (V->vptr && V->vsrc)),
               "space");
  FLOW_REQUIRE(V->r1 == 0, "forms of arguments on strips");
  return FLOW_OK;
}

// The instance of a form kernel is chosen here and nowhere else: launch(NF,
// EXT) is called with the number of the form's fields (0..6) and whether its
// program holds an extended opcode, as std::integral_constants; it launches
// the one kernel <NF(), ..., EXT()>.
template <int N>
using Int = std::integral_constant<int, N>;

template <class Launch>
static int dispatch_form(const flow_form* F, Launch&& launch) {
  const bool ext = form_is_extended(F);
  const auto with_ext = [&](auto NF) {
    if (ext) launch(NF, std::true_type{});
    else launch(NF, std::false_type{});
  };
  switch (F->nfield) {
    case 0: with_ext(Int<0>{}); break;
    case 1: with_ext(Int<1>{}); break;
    case 2: with_ext(Int<2>{}); break;
    case 3: with_ext(Int<3>{}); break;
    case 4: with_ext(Int<4>{}); break;
    case 5: with_ext(Int<5>{}); break;
    default: with_ext(Int<6>{}); break;
  }
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// ... and launch(NF, EXT, DEG) for the kernels of a space of degree 1 or 2
template <class Launch>
static int dispatch_form(const flow_form* F, int deg, Launch&& launch) {
  if (deg == 1)
    return dispatch_form(F, [&](auto NF, auto EXT) { launch(NF, EXT, Int<1>{}); });
  return dispatch_form(F, [&](auto NF, auto EXT) { launch(NF, EXT, Int<2>{}); });
}

// td = 0: the functional; the degree of the space: the load vector
static int launch_cells(const flow_mesh* mesh, const flow_form* F, int td, int cb, int ce,
                        double* scratch, hipStream_t st) {
  const dim3 grid((ce - cb + kBlock - 1) / kBlock);
  const auto launch = [&](auto NF, auto EXT, auto TD) {
    hipLaunchKernelGGL((form_cell_kernel<NF(), TD(), EXT()>), grid, dim3(kBlock), 0, st,
                       mesh->nc, cb, ce, mesh->xy, *F, scratch);
  };
  if (td == 0)
    return dispatch_form(F, [&](auto NF, auto EXT) { launch(NF, EXT, Int<0>{}); });
  return dispatch_form(F, td, launch);
}

static int launch_facets(const flow_mesh* mesh, const flow_form* F, int nfacets,
                         const int* fcell, const int* flocal, double* scratch,
                         hipStream_t st) {
  const dim3 grid((nfacets + kBlock - 1) / kBlock);
  return dispatch_form(F, [&](auto NF, auto EXT) {
    hipLaunchKernelGGL((form_facet_kernel<NF(), EXT()>), grid, dim3(kBlock), 0, st,
                       mesh->nc, nfacets, fcell, flocal, mesh->xy, *F, scratch);
  });
}

static int launch_interior_facets(const flow_mesh* mesh, const flow_form* F, int nfacets,
                                  const int* fplus, const int* lplus, const int* fother,
                                  int minus_slots, double* out, hipStream_t st) {
  const dim3 grid((nfacets + kBlock - 1) / kBlock);
  return dispatch_form(F, [&](auto NF, auto EXT) {
    hipLaunchKernelGGL((form_interior_facet_kernel<NF(), EXT()>), grid, dim3(kBlock), 0,
                       st, mesh->nc, nfacets, fplus, lplus, fother, minus_slots,
                       mesh->xy, *F, out);
  });
}

static int launch_facet_values(const flow_mesh* mesh, const flow_form* F, int nfacets,
                               const int* fcell, const int* flocal, const int* fdest,
                               const int* fflip, double* values, double* integrals,
                               hipStream_t st) {
  const dim3 grid((nfacets * F->nq + kBlock - 1) / kBlock);
  return dispatch_form(F, [&](auto NF, auto EXT) {
    hipLaunchKernelGGL((form_facet_values_kernel<NF(), EXT()>), grid, dim3(kBlock), 0, st,
                       mesh->nc, nfacets, fcell, flocal, fdest, fflip, mesh->xy, *F,
                       values, integrals);
  });
}

static int launch_points(const flow_mesh* mesh, const flow_form* F, int n,
                         const int* cell, const double* bary, double* out,
                         hipStream_t st) {
  const dim3 grid((n + kBlock - 1) / kBlock);
  return dispatch_form(F, [&](auto NF, auto EXT) {
    hipLaunchKernelGGL((form_points_kernel<NF(), EXT()>), grid, dim3(kBlock), 0, st,
                       mesh->nc, mesh->xy, *F, n, cell, bary, out);
  });
}

// the element kernels of a form of arguments on a space of degree deg
enum class Element { matrix, vector, newton };

static int launch_element(Element what, const flow_mesh* mesh, int deg,
                          const flow_form* F, int live, double* scratch, hipStream_t st) {
  const dim3 grid((mesh->nc + kBlock - 1) / kBlock);
  switch (what) {
    case Element::matrix:
      return dispatch_form(F, deg, [&](auto NF, auto EXT, auto DEG) {
        hipLaunchKernelGGL((form_matrix_kernel<NF(), DEG(), EXT()>), grid, dim3(kBlock), 0,
                           st, mesh->nc, mesh->xy, *F, live, scratch);
      });
    case Element::vector:
      return dispatch_form(F, deg, [&](auto NF, auto EXT, auto DEG) {
        hipLaunchKernelGGL((form_vector_kernel<NF(), DEG(), EXT()>), grid, dim3(kBlock), 0,
                           st, mesh->nc, mesh->xy, *F, live, scratch);
      });
    default:
      return dispatch_form(F, deg, [&](auto NF, auto EXT, auto DEG) {
        hipLaunchKernelGGL((form_newton_kernel<NF(), DEG(), EXT()>), grid, dim3(kBlock), 0,
                           st, mesh->nc, mesh->xy, *F, live, scratch);
      });
  }
}

template <int RANK>
static int launch_facet_arguments(const flow_mesh* mesh, int deg, const flow_form* F,
                                  int live, int nfacets, const int* fcell,
                                  const int* flocal, double* scratch, hipStream_t st) {
  const dim3 grid((nfacets * (deg == 1 ? 3 : 6) + kBlock - 1) / kBlock);
  return dispatch_form(F, deg, [&](auto NF, auto EXT, auto DEG) {
    hipLaunchKernelGGL((form_facet_arguments_kernel<NF(), DEG(), EXT(), RANK>), grid,
                       dim3(kBlock), 0, st, mesh->nc, nfacets, fcell, flocal, mesh->xy, *F,
                       live, scratch);
  });
}

// flow_form_facet_matrix (RANK 2) / flow_form_facet_vector (RANK 1)
template <int RANK>
static int facet_arguments(const flow_mesh* mesh, const flow_space* V,
                           const flow_form* form, int nfacets, const int* facet_cell,
                           const int* facet_local, int ntargets, const int* map_targets,
                           const int* map_ptr, const int* map_src, double* scratch,
                           double* out, void* stream) {
  // (the gather runs over the facet map, not over the space's own maps: the
  // helper asks for neither, and the second "space" requirement adds what
  // this entry point needs of the space instead)
  int rc = check_argument_space(mesh, V, false, false);
  if (rc) return rc;
  FLOW_REQUIRE((RANK == 1 || V->nnz > 0) && V->cell_dofs, "space");
  int live = 0;
  if ((rc = check_form(form, 3, true, false, RANK == 2 ? FLOW_FORM_SLOTS : 3, &live)))
    return rc;
  FLOW_REQUIRE(nfacets >= 0 && ntargets >= 0, "facet / target count");
  if (nfacets == 0 || ntargets == 0) return FLOW_OK;
  const int nl = V->deg == 1 ? 3 : 6;
  const long long nsrc = static_cast<long long>(nfacets) * nl * (RANK == 2 ? nl : 1);
  FLOW_REQUIRE(nsrc < (1LL << 31) - kBlock, "facet count (scratch entries)");
  FLOW_REQUIRE(ntargets <= (RANK == 2 ? V->nnz : V->n) && ntargets <= nsrc,
               "target count");
  FLOW_REQUIRE(facet_cell && facet_local, "facet lists");
  FLOW_REQUIRE(map_targets && map_ptr && map_src, "facet contribution map");
  FLOW_REQUIRE(scratch && out, "pointers");
  hipStream_t st = as_stream(stream);
  if ((rc = launch_facet_arguments<RANK>(mesh, V->deg, form, live, nfacets, facet_cell,
                                         facet_local, scratch, st)))
    return rc;
  hipLaunchKernelGGL(facet_gather_kernel, dim3((ntargets + kBlock - 1) / kBlock),
                     dim3(kBlock), 0, st, ntargets, map_targets, map_ptr, map_src,
                     static_cast<int>(nsrc), scratch, RANK == 2 ? V->nnz : V->n, out);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

template <bool BY_CELL>
static int launch_cell_list(const flow_mesh* mesh, const flow_form* F, int ncells,
                            const int* cells, double* out, hipStream_t st) {
  const dim3 grid((ncells + kBlock - 1) / kBlock);
  return dispatch_form(F, [&](auto NF, auto EXT) {
    hipLaunchKernelGGL((form_cells_kernel<NF(), EXT(), BY_CELL>), grid, dim3(kBlock), 0, st,
                       mesh->nc, ncells, cells, mesh->xy, *F, out);
  });
}

// what the two rank-0 cell-list entry points ask
static int check_cell_list(const flow_mesh* mesh, const flow_form* form, int ncells) {
  int rc = check_form_mesh(mesh);
  if (rc) return rc;
  FLOW_REQUIRE(mesh->c1 == 0, "cell subdomains on strips");
  if ((rc = check_form(form))) return rc;
  FLOW_REQUIRE(form->nout == 1, "a functional has one output");
  FLOW_REQUIRE(ncells >= 0, "cell count");
  return FLOW_OK;
}

// flow_form_cells_matrix (RANK 2) / flow_form_cells_vector (RANK 1)
template <int RANK>
static int cells_arguments(const flow_mesh* mesh, const flow_space* V,
                           const flow_form* form, int ncells, const int* cells,
                           int ntargets, const int* map_targets, const int* map_ptr,
                           const int* map_src, double* scratch, double* out,
                           void* stream) {
  // (the gather runs over the cell map, not over the space's own maps, as in
  // facet_arguments)
  int rc = check_argument_space(mesh, V, false, false);
  if (rc) return rc;
  FLOW_REQUIRE((RANK == 1 || V->nnz > 0) && V->cell_dofs, "space");
  int live = 0;
  if ((rc = check_form(form, 1, false, false, RANK == 2 ? FLOW_FORM_SLOTS : 3, &live)))
    return rc;
  FLOW_REQUIRE(ncells >= 0 && ntargets >= 0, "cell / target count");
  if (ncells == 0 || ntargets == 0) return FLOW_OK;
  const int nl = V->deg == 1 ? 3 : 6;
  const long long nsrc = static_cast<long long>(ncells) * nl * (RANK == 2 ? nl : 1);
  FLOW_REQUIRE(nsrc < (1LL << 31) - kBlock, "cell count (scratch entries)");
  FLOW_REQUIRE(ntargets <= (RANK == 2 ? V->nnz : V->n) && ntargets <= nsrc,
               "target count");
  FLOW_REQUIRE(cells, "cell list");
  FLOW_REQUIRE(map_targets && map_ptr && map_src, "cell contribution map");
  FLOW_REQUIRE(scratch && out, "pointers");
  hipStream_t st = as_stream(stream);
  const dim3 grid((ncells + kBlock - 1) / kBlock);
  if constexpr (RANK == 2) {
    rc = dispatch_form(form, V->deg, [&](auto NF, auto EXT, auto DEG) {
      hipLaunchKernelGGL((form_cells_matrix_kernel<NF(), DEG(), EXT()>), grid, dim3(kBlock),
                         0, st, mesh->nc, ncells, cells, mesh->xy, *form, live, scratch);
    });
  } else {
    rc = dispatch_form(form, V->deg, [&](auto NF, auto EXT, auto DEG) {
      hipLaunchKernelGGL((form_cells_vector_kernel<NF(), DEG(), EXT()>), grid, dim3(kBlock),
                         0, st, mesh->nc, ncells, cells, mesh->xy, *form, live, scratch);
    });
  }
  if (rc) return rc;
  hipLaunchKernelGGL(facet_gather_kernel, dim3((ntargets + kBlock - 1) / kBlock),
                     dim3(kBlock), 0, st, ntargets, map_targets, map_ptr, map_src,
                     static_cast<int>(nsrc), scratch, RANK == 2 ? V->nnz : V->n, out);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// ---------------------------------------------------------------------------
// Rectangular blocks (forms.py, mixed_arguments: the velocity-pressure
// coupling of a Taylor-Hood form): a test function of degree DT and a trial
// function of degree DS.  form_matrix_kernel, form_facet_arguments_kernel
// (RANK 2) and form_cells_matrix_kernel with two bases: per point and test
// derivative b, t_j = sum_a w c_ba D_a psi_j over the TRIAL basis first, then
// Ke[i][j] += D_b phi_i t_j over the TEST basis; the program, the slots, the
// live mask, the walk over the rule and the form_point_n call are theirs.
// They are kernels of their own, not a parameter of those: those are short of
// scalar registers, and their instances stay as they are.  With DT == DS one
// basis is tabulated and the arithmetic is add_matrix_terms': the bits of the
// square kernel.  Ke goes to scratch[(i*NLS + j)*n + k], n the cells | facets |
// list entries, k fastest.
// ---------------------------------------------------------------------------
template <int NLT, int NLS, int NS>
__device__ __forceinline__ void add_rect_terms(int m, double w, const double (&slots)[NS],
                                               const double (&phi)[NLT],
                                               const double (&gphi)[NLT][2],
                                               const double (&psi)[NLS],
                                               const double (&gpsi)[NLS][2],
                                               double (&Ke)[NLT][NLS]) {
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    if (((m >> (3 * b)) & 7) == 0) continue;
    double t[NLS];
    trial_sums<NLS>(m, 3 * b, w, slots, psi, gpsi, t);
#pragma unroll
    for (int i = 0; i < NLT; ++i) {
      const double di = arg_basis<NLT>(b, phi, gphi, i);
#pragma unroll
      for (int j = 0; j < NLS; ++j) Ke[i][j] += di * t[j];
    }
  }
}

// one point of a cell: both bases at L, then add_rect_terms
template <int DT, int DS, int NS>
__device__ __forceinline__ void rect_point(const Geom& g, const double (&L)[3], int m,
                                           double w, const double (&slots)[NS],
                                           double (&Ke)[Elem<DT>::NL][Elem<DS>::NL]) {
  constexpr int NLT = Elem<DT>::NL, NLS = Elem<DS>::NL;
  double phi[NLT], dphi[NLT][3], gphi[NLT][2];
  basis<DT>(L, phi, dphi);
  phys_grad<NLT>(g, dphi, gphi);
  if constexpr (DT == DS) {
    add_rect_terms<NLT, NLS>(m, w, slots, phi, gphi, phi, gphi, Ke);
  } else {
    double psi[NLS], dpsi[NLS][3], gpsi[NLS][2];
    basis<DS>(L, psi, dpsi);
    phys_grad<NLS>(g, dpsi, gpsi);
    add_rect_terms<NLT, NLS>(m, w, slots, phi, gphi, psi, gpsi, Ke);
  }
}

// cell c (LIST: cells[k]) of n = nc (LIST: nsel) lanes
template <int NF, int DT, int DS, bool EXT, bool LIST>
__global__ __launch_bounds__(kBlock) void form_rect_matrix_kernel(
    int nc, int n, const int* __restrict__ cells, const double* __restrict__ xy,
    const flow_form F, int live, double* __restrict__ scratch) {
  constexpr int NLT = Elem<DT>::NL, NLS = Elem<DS>::NL;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  double* const dst = scratch + k;
  int c = k;
  if constexpr (LIST) {
    c = cells[k];
    if (c < 0 || c >= nc) {
#pragma unroll
      for (int ij = 0; ij < NLT * NLS; ++ij)
        dst[static_cast<size_t>(ij) * n] = __builtin_nan("");
      return;
    }
  }
  FormCell<NF> C;
  load_form_cell<NF>(F, nc, xy, c, C);
  double Ke[NLT][NLS];
#pragma unroll
  for (int i = 0; i < NLT; ++i)
#pragma unroll
    for (int j = 0; j < NLS; ++j) Ke[i][j] = 0.0;
  for (int q = 0; q < F.nq; ++q) {
    const double xi = F.rule[3 * q], eta = F.rule[3 * q + 1];
    const double w = F.rule[3 * q + 2] * C.g.adet;
    const double L[3] = {1.0 - xi - eta, xi, eta};
    FormSlots<FLOW_FORM_SLOTS> out;
#pragma unroll
    for (int s = 0; s < FLOW_FORM_SLOTS; ++s) out.v[s] = 0.0;
    form_point_n<NF, false, EXT>(F, C.U, C.X, C.Y, C.g, L, q, nc, c, 0.0, 0.0, out);
    // (the mask through an empty asm, as in form_matrix_kernel)
    int m = live;
    asm volatile("" : "+s"(m));
    rect_point<DT, DS>(C.g, L, m, w, out.v, Ke);
  }
#pragma unroll
  for (int i = 0; i < NLT; ++i)
#pragma unroll
    for (int j = 0; j < NLS; ++j)
      dst[static_cast<size_t>(i * NLS + j) * n] = Ke[i][j];
}

// one lane per (local test dof i < NLT, facet k), k fastest: row i of the
// facet's element matrix, as form_facet_arguments_kernel (RANK 2) writes it
template <int NF, int DT, int DS, bool EXT>
__global__ __launch_bounds__(kBlock) void form_rect_facet_kernel(
    int nc, int nfacets, const int* __restrict__ fcell,
    const int* __restrict__ flocal, const double* __restrict__ xy,
    const flow_form F, int live, double* __restrict__ scratch) {
  constexpr int NLT = Elem<DT>::NL, NLS = Elem<DS>::NL;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nfacets * NLT) return;
  const int i = idx / nfacets, k = idx - i * nfacets;
  double* const dst = scratch + static_cast<size_t>(i) * NLS * nfacets + k;
  const int c = fcell[k], lf = flocal[k];
  if (c < 0 || c >= nc || lf < 0 || lf > 2) {
#pragma unroll
    for (int j = 0; j < NLS; ++j)
      dst[static_cast<size_t>(j) * nfacets] = __builtin_nan("");
    return;
  }
  FormCell<NF> C;
  load_form_cell<NF>(F, nc, xy, c, C);
  const FacetFrame f = facet_frame(C.g, lf);
  double acc[NLS];
#pragma unroll
  for (int j = 0; j < NLS; ++j) acc[j] = 0.0;
  for (int q = 0; q < F.nq; ++q) {
    const int row = lf * F.nq + q;
    const double xi = F.rule[3 * row], eta = F.rule[3 * row + 1];
    const double w = F.rule[3 * row + 2] * f.len;
    const double L[3] = {1.0 - xi - eta, xi, eta};
    FormSlots<FLOW_FORM_SLOTS> out;
#pragma unroll
    for (int s = 0; s < FLOW_FORM_SLOTS; ++s) out.v[s] = 0.0;
    form_point_n<NF, true, EXT>(F, C.U, C.X, C.Y, C.g, L, row, nc, c, f.n0, f.n1, out);
    double phi[NLT], dphi[NLT][3], gphi[NLT][2];
    basis<DT>(L, phi, dphi);
    phys_grad<NLT>(C.g, dphi, gphi);
    double psi[NLS], dpsi[NLS][3], gpsi[NLS][2];
    basis<DS>(L, psi, dpsi);
    phys_grad<NLS>(C.g, dpsi, gpsi);
    // (the mask through an empty asm, as in form_matrix_kernel)
    int m = live;
    asm volatile("" : "+s"(m));
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      if (((m >> (3 * b)) & 7) == 0) continue;
      const double di = own_basis<NLT>(b, phi, gphi, i);
      double t[NLS];
      trial_sums<NLS>(m, 3 * b, w, out.v, psi, gpsi, t);
#pragma unroll
      for (int j = 0; j < NLS; ++j) acc[j] += di * t[j];
    }
  }
#pragma unroll
  for (int j = 0; j < NLS; ++j) dst[static_cast<size_t>(j) * nfacets] = acc[j];
}

// vals[e] = sum of scratch[src[t]], t in [ptr[e], ptr[e+1]), in that order (the
// order and grouping of gather_kernel: adding its padding zeros changes no
// bit).  A row of ptr or an entry of src outside the scratch gives NaN, not a
// stray read.  No atomics: two calls give the same bits.
__global__ __launch_bounds__(kBlock) void rect_gather_kernel(
    int nnz, const int* __restrict__ ptr, const int* __restrict__ src, int nsrc,
    const double* __restrict__ scratch, double* __restrict__ vals) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  const int a = ptr[e], b = ptr[e + 1];
  double s = 0.0;
  if (a < 0 || b > nsrc || a > b) {
    s = __builtin_nan("");
  } else {
    for (int t = a; t < b; ++t) {
      const int x = src[t];
      s += (x >= 0 && x < nsrc) ? scratch[x] : __builtin_nan("");
    }
  }
  vals[e] = s;
}

// vals[e] = 0 where the row or the column of entry e is a Dirichlet dof: one
// lane per row, plain vector stores
__global__ __launch_bounds__(kBlock) void bc_rect_mask_kernel(
    int n_rows, const int* __restrict__ rowptr, const int* __restrict__ cols,
    const unsigned char* __restrict__ row_isbc,
    const unsigned char* __restrict__ col_isbc, double* __restrict__ vals) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const bool rb = row_isbc[r] != 0;
  for (int e = rowptr[r]; e < rowptr[r + 1]; ++e)
    if (rb || col_isbc[cols[e]]) vals[e] = 0.0;
}

// launch(NF, EXT, DT, DS) for the kernels of a (test, trial) pair of degrees
template <class Launch>
static int dispatch_rect(const flow_form* F, int dt, int ds, Launch&& launch) {
  return dispatch_form(F, dt, [&](auto NF, auto EXT, auto DT) {
    if (ds == 1) launch(NF, EXT, DT, Int<1>{});
    else launch(NF, EXT, DT, Int<2>{});
  });
}

// what the three rectangular entry points ask of the mesh, the two spaces and
// the program (rows = 1: cells, 3: facets, where NORMAL is legal).  Each dof of
// a space on this mesh lies in a cell, so n <= nloc * nc: a space with more
// belongs to another mesh.
static int check_rect(const flow_mesh* mesh, const flow_space* Vt, const flow_space* Vs,
                      const flow_form* form, int rows, int* live) {
  int rc = check_form_mesh(mesh);
  if (rc) return rc;
  FLOW_REQUIRE(mesh->c1 == 0, "rectangular forms on strips");
  FLOW_REQUIRE(Vt && Vs, "spaces");
  FLOW_REQUIRE((Vt->deg == 1 || Vt->deg == 2) && (Vs->deg == 1 || Vs->deg == 2),
               "space degree (1 or 2)");
  FLOW_REQUIRE(Vt->r1 == 0 && Vs->r1 == 0, "rectangular forms on strips");
  FLOW_REQUIRE(Vt->n > 0 && Vs->n > 0 &&
                   Vt->n <= static_cast<long long>(Vt->deg == 1 ? 3 : 6) * mesh->nc &&
                   Vs->n <= static_cast<long long>(Vs->deg == 1 ? 3 : 6) * mesh->nc,
               "space (of another mesh)");
  return check_form(form, rows, rows == 3, false, FLOW_FORM_SLOTS, live);
}

static int rect_matrix(const flow_mesh* mesh, const flow_space* Vt, const flow_space* Vs,
                       const flow_form* form, double* scratch, double* vals,
                       const int* cptr, const int* csrc, int nnz, void* stream) {
  int live = 0;
  int rc = check_rect(mesh, Vt, Vs, form, 1, &live);
  if (rc) return rc;
  const long long nsrc = static_cast<long long>(mesh->nc) * (Vt->deg == 1 ? 3 : 6) *
                         (Vs->deg == 1 ? 3 : 6);
  FLOW_REQUIRE(nsrc < (1LL << 31) - kBlock, "cell count (scratch entries)");
  FLOW_REQUIRE(nnz > 0 && nnz <= nsrc &&
                   nnz <= static_cast<long long>(Vt->n) * Vs->n,
               "nnz (more entries than the scratch or the block holds)");
  FLOW_REQUIRE(scratch && vals && cptr && csrc, "pointers");
  hipStream_t st = as_stream(stream);
  const dim3 grid((mesh->nc + kBlock - 1) / kBlock);
  rc = dispatch_rect(form, Vt->deg, Vs->deg, [&](auto NF, auto EXT, auto DT, auto DS) {
    hipLaunchKernelGGL((form_rect_matrix_kernel<NF(), DT(), DS(), EXT(), false>), grid,
                       dim3(kBlock), 0, st, mesh->nc, mesh->nc,
                       static_cast<const int*>(nullptr), mesh->xy, *form, live, scratch);
  });
  if (rc) return rc;
  hipLaunchKernelGGL(rect_gather_kernel, dim3((nnz + kBlock - 1) / kBlock), dim3(kBlock), 0,
                     st, nnz, cptr, csrc, static_cast<int>(nsrc), scratch, vals);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// FACET: n facets (cells = facet_cell, local = facet_local), else n listed cells
template <bool FACET>
static int rect_list(const flow_mesh* mesh, const flow_space* Vt, const flow_space* Vs,
                     const flow_form* form, int n, const int* cells, const int* local,
                     int ntargets, const int* map_targets, const int* map_ptr,
                     const int* map_src, double* scratch, double* vals, int nnz,
                     void* stream) {
  int live = 0;
  int rc = check_rect(mesh, Vt, Vs, form, FACET ? 3 : 1, &live);
  if (rc) return rc;
  FLOW_REQUIRE(n >= 0 && ntargets >= 0, "list / target count");
  if (n == 0 || ntargets == 0) return FLOW_OK;
  const int nlt = Vt->deg == 1 ? 3 : 6;
  const long long nsrc = static_cast<long long>(n) * nlt * (Vs->deg == 1 ? 3 : 6);
  FLOW_REQUIRE(nsrc < (1LL << 31) - kBlock, "list length (scratch entries)");
  FLOW_REQUIRE(nnz > 0 && nnz <= static_cast<long long>(Vt->n) * Vs->n, "nnz");
  FLOW_REQUIRE(ntargets <= nnz && ntargets <= nsrc, "target count");
  FLOW_REQUIRE(cells && (!FACET || local), "cell / facet lists");
  FLOW_REQUIRE(map_targets && map_ptr && map_src, "contribution map");
  FLOW_REQUIRE(scratch && vals, "pointers");
  hipStream_t st = as_stream(stream);
  if constexpr (FACET) {
    const dim3 grid((n * nlt + kBlock - 1) / kBlock);
    rc = dispatch_rect(form, Vt->deg, Vs->deg, [&](auto NF, auto EXT, auto DT, auto DS) {
      hipLaunchKernelGGL((form_rect_facet_kernel<NF(), DT(), DS(), EXT()>), grid,
                         dim3(kBlock), 0, st, mesh->nc, n, cells, local, mesh->xy, *form,
                         live, scratch);
    });
  } else {
    const dim3 grid((n + kBlock - 1) / kBlock);
    rc = dispatch_rect(form, Vt->deg, Vs->deg, [&](auto NF, auto EXT, auto DT, auto DS) {
      hipLaunchKernelGGL((form_rect_matrix_kernel<NF(), DT(), DS(), EXT(), true>), grid,
                         dim3(kBlock), 0, st, mesh->nc, n, cells, mesh->xy, *form, live,
                         scratch);
    });
  }
  if (rc) return rc;
  hipLaunchKernelGGL(facet_gather_kernel, dim3((ntargets + kBlock - 1) / kBlock),
                     dim3(kBlock), 0, st, ntargets, map_targets, map_ptr, map_src,
                     static_cast<int>(nsrc), scratch, nnz, vals);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// ---------------------------------------------------------------------------
// Forms of arguments on a vector space (forms.py, vector_arguments): the table
// of such a form is one scalar table per block (r, s) = (test, trial
// component), compiled to the programs of a scalar form.  Every program runs
// on the instances of form_matrix_kernel / form_vector_kernel that a scalar
// form launches, into the scratch plane of its block; ONE gather then sums
// the planes of all blocks into the value planes of a kind-2 operator (rank
// 2) or into the two components of the vector (rank 1).
// ---------------------------------------------------------------------------
// offset of the scratch plane of block p in doubles; < 0: the block is absent
struct BlockPlanes {
  long long off[4];
};

// s[p] = sum of scratch[off[p] + src[e]], e in [a, b), for NP planes over one
// index list: added in that order from 0.0 as gather_kernel adds them (the
// same bits); 0.0 for an absent plane
template <int NP>
__device__ __forceinline__ void block_sum(const int* __restrict__ src, int a, int b,
                                          const double* __restrict__ scratch,
                                          const long long* off, double (&s)[NP]) {
#pragma unroll
  for (int p = 0; p < NP; ++p) s[p] = 0.0;
  for (int t = a; t < b; t += 4) {
    int idx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) idx[j] = t + j < b ? src[t + j] : -1;
    double w[NP][4];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        w[p][j] = (off[p] >= 0 && idx[j] >= 0) ? scratch[off[p] + idx[j]] : 0.0;
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int j = 0; j < 4; ++j) s[p] += w[p][j];
  }
}

// out[p*out_stride + k] = block_sum over [ptr[k], ptr[k+1]) of plane p
template <int NP>
__global__ __launch_bounds__(kBlock) void block_gather_kernel(
    int nout, const int* __restrict__ ptr, const int* __restrict__ src,
    const double* __restrict__ scratch, const BlockPlanes P, size_t out_stride,
    double* __restrict__ out) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nout;
       k += gridDim.x * blockDim.x) {
    double s[NP];
    block_sum<NP>(src, ptr[k], ptr[k + 1], scratch, P.off, s);
#pragma unroll
    for (int p = 0; p < NP; ++p) out[static_cast<size_t>(p) * out_stride + k] = s[p];
  }
}

// dst += src, entry by entry: a further program of a block that has one
__global__ __launch_bounds__(kBlock) void plane_add_kernel(
    size_t n, const double* __restrict__ src, double* __restrict__ dst) {
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * blockDim.x)
    dst[i] += src[i];
}

// One element kernel of a block form: the first program of a block writes
// the block's own plane, a further one the spare plane, which is then added
// to the own one.
static int launch_block_program(Element what, const flow_mesh* mesh, int deg,
                                const flow_form* F, int live, bool first, double* own,
                                double* spare, size_t plane, hipStream_t st) {
  const int rc = launch_element(what, mesh, deg, F, live, first ? own : spare, st);
  if (rc || first) return rc;
  hipLaunchKernelGGL(plane_add_kernel, dim3(grid_for(plane, kBlock, 1 << 20)),
                     dim3(kBlock), 0, st, plane, spare, own);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// flow_form_block_matrix (RANK 2) / flow_form_block_vector (RANK 1)
template <int RANK>
static int block_arguments(const flow_mesh* mesh, const flow_space* V, int nprog,
                           const flow_form* forms, const int* blocks, double* scratch,
                           double* out, size_t out_stride, void* stream) {
  constexpr int NB = RANK == 2 ? 4 : 2;
  int rc = check_argument_space(mesh, V, RANK == 2, RANK == 1);
  if (rc) return rc;
  FLOW_REQUIRE(nprog >= 1 && nprog <= 64 && forms && blocks, "block programs");
  FLOW_REQUIRE(scratch && out, "pointers");
  FLOW_REQUIRE(out_stride >= static_cast<size_t>(RANK == 2 ? V->nnz : V->n),
               "plane stride");
  int live[64];
  int count[NB] = {};
  for (int k = 0; k < nprog; ++k) {
    FLOW_REQUIRE(blocks[k] >= 0 && blocks[k] < NB, "block tag");
    if ((rc = check_form(forms + k, 1, false, false, RANK == 2 ? FLOW_FORM_SLOTS : 3,
                         live + k)))
      return rc;
    ++count[blocks[k]];
  }
  // the scratch planes: one per present block, in the order of p, and one
  // more behind them where a block has several programs
  const int nl = V->deg == 1 ? 3 : 6;
  const size_t plane = static_cast<size_t>(RANK == 2 ? nl * nl : nl) * mesh->nc;
  BlockPlanes P;
  int npresent = 0;
  for (int p = 0; p < 4; ++p)
    P.off[p] = (p < NB && count[p] > 0) ? static_cast<long long>(plane * npresent++) : -1;
  double* const spare = scratch + plane * npresent;
  hipStream_t st = as_stream(stream);
  int seen[NB] = {};
  for (int k = 0; k < nprog; ++k) {
    const int p = blocks[k];
    if ((rc = launch_block_program(RANK == 2 ? Element::matrix : Element::vector, mesh,
                                   V->deg, forms + k, live[k], seen[p]++ == 0,
                                   scratch + P.off[p], spare, plane, st)))
      return rc;
  }
  const int nout = RANK == 2 ? V->nnz : V->n;
  const int* ptr = RANK == 2 ? V->cptr : V->vptr;
  const int* src = RANK == 2 ? V->csrc : V->vsrc;
  hipLaunchKernelGGL(block_gather_kernel<NB>, dim3(grid_for(nout, kBlock, 1 << 20)),
                     dim3(kBlock), 0, st, nout, ptr, src, scratch, P, out_stride, out);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

// ---------------------------------------------------------------------------
// Block Newton (flow_form_block_newton): the Jacobian of a residual on a vector
// space is a 2x2-block form, the residual a 2-component one.  A job
// newton(p) runs the form_newton_kernel instance of a scalar Newton pass for
// block p = 2 r + s TOGETHER with residual component r -- they share the test
// basis and the subtrees in u and grad u --, a job matrix(p) / vector(r) the
// form_matrix_kernel / form_vector_kernel instance a block form launches.  ONE
// gather then sums all of it: lanes [0, nnz) the four value planes over cptr /
// csrc, lanes [nnz, nnz + n) the two vector components over vptr / vsrc.
// ---------------------------------------------------------------------------
// offsets of the scratch planes in doubles, < 0: absent.  mat[p]: Ke of block
// p; vec[r]: be of component r (behind Ke of its block where a newton job
// wrote it: form_newton_kernel puts be there)
struct NewtonPlanes {
  long long mat[4];
  long long vec[2];
};

// vals[p*vals_stride + k], k < nnz, and b[r*n + i], i < n, in one launch;
// consecutive lanes take consecutive k (i): the stores coalesce, the index
// loads run over neighbouring rows of cptr / csrc (vptr / vsrc)
__global__ __launch_bounds__(kBlock) void block_newton_gather_kernel(
    int nnz, int n, const int* __restrict__ cptr, const int* __restrict__ csrc,
    const int* __restrict__ vptr, const int* __restrict__ vsrc,
    const double* __restrict__ scratch, const NewtonPlanes P, size_t vals_stride,
    double* __restrict__ vals, double* __restrict__ b) {
  const long long total = static_cast<long long>(nnz) + n;
  for (long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
       k < total; k += static_cast<long long>(gridDim.x) * blockDim.x) {
    if (k < nnz) {
      double s[4];
      block_sum<4>(csrc, cptr[k], cptr[k + 1], scratch, P.mat, s);
#pragma unroll
      for (int p = 0; p < 4; ++p) vals[static_cast<size_t>(p) * vals_stride + k] = s[p];
    } else {
      const int i = static_cast<int>(k - nnz);
      double s[2];
      block_sum<2>(vsrc, vptr[i], vptr[i + 1], scratch, P.vec, s);
#pragma unroll
      for (int r = 0; r < 2; ++r) b[static_cast<size_t>(r) * n + i] = s[r];
    }
  }
}

static int block_newton(const flow_mesh* mesh, const flow_space* V, int nprog,
                        const flow_form* forms, const int* kinds, const int* tags,
                        double* scratch, size_t nscratch, double* vals,
                        size_t plane_stride, double* b, void* stream) {
  int rc = check_argument_space(mesh, V, true, true);
  if (rc) return rc;
  FLOW_REQUIRE(nprog >= 1 && nprog <= 64 && forms && kinds && tags, "block programs");
  FLOW_REQUIRE(scratch && vals && b, "pointers");
  FLOW_REQUIRE(plane_stride >= static_cast<size_t>(V->nnz), "plane stride");
  int live[64];
  int nmat[4] = {}, nvec[2] = {};
  bool newton_mat[4] = {}, newton_vec[2] = {};
  for (int k = 0; k < nprog; ++k) {
    const int kind = kinds[k], tag = tags[k];
    FLOW_REQUIRE(kind >= FLOW_BLOCK_NEWTON && kind <= FLOW_BLOCK_VECTOR, "block job kind");
    FLOW_REQUIRE(tag >= 0 && tag < (kind == FLOW_BLOCK_VECTOR ? 2 : 4), "block tag");
    if ((rc = check_form(forms + k, 1, false, false,
                         kind == FLOW_BLOCK_NEWTON   ? FLOW_FORM_NEWTON_SLOTS
                         : kind == FLOW_BLOCK_MATRIX ? FLOW_FORM_SLOTS
                                                     : 3,
                         live + k)))
      return rc;
    if (kind == FLOW_BLOCK_NEWTON) {
      // (Ke and be of a newton job go straight to the planes of the block
      // and the component: it is the first program of both)
      FLOW_REQUIRE(nmat[tag] == 0 && nvec[tag >> 1] == 0,
                   "a newton job is the first program of its block and component");
      newton_mat[tag] = newton_vec[tag >> 1] = true;
    }
    if (kind != FLOW_BLOCK_VECTOR) ++nmat[tag];
    if (kind != FLOW_BLOCK_MATRIX) ++nvec[kind == FLOW_BLOCK_VECTOR ? tag : tag >> 1];
  }
  // the scratch planes: per block with a program nl*nl*nc doubles, in the
  // order of p, a newton job's nl*nc of be directly behind its Ke; then the
  // components no newton job writes; then one spare plane where a block or a
  // component has several programs
  const int nl = V->deg == 1 ? 3 : 6;
  const size_t mplane = static_cast<size_t>(nl) * nl * mesh->nc;
  const size_t vplane = static_cast<size_t>(nl) * mesh->nc;
  NewtonPlanes P;
  size_t cur = 0;
  for (int r = 0; r < 2; ++r) P.vec[r] = -1;
  for (int p = 0; p < 4; ++p) {
    P.mat[p] = -1;
    if (nmat[p] == 0) continue;
    P.mat[p] = static_cast<long long>(cur);
    cur += mplane;
    if (newton_mat[p]) {
      P.vec[p >> 1] = static_cast<long long>(cur);
      cur += vplane;
    }
  }
  for (int r = 0; r < 2; ++r)
    if (nvec[r] > 0 && !newton_vec[r]) {
      P.vec[r] = static_cast<long long>(cur);
      cur += vplane;
    }
  double* const spare = scratch + cur;
  bool mspare = false, vspare = false;
  for (int p = 0; p < 4; ++p) mspare = mspare || nmat[p] > 1;
  for (int r = 0; r < 2; ++r) vspare = vspare || nvec[r] > 1;
  cur += mspare ? mplane : vspare ? vplane : 0;
  FLOW_REQUIRE(cur <= nscratch, "scratch size");
  hipStream_t st = as_stream(stream);
  int mseen[4] = {}, vseen[2] = {};
  for (int k = 0; k < nprog; ++k) {
    const int kind = kinds[k], tag = tags[k];
    const flow_form* F = forms + k;
    if (kind == FLOW_BLOCK_NEWTON) {
      ++mseen[tag];
      ++vseen[tag >> 1];
      if ((rc = launch_element(Element::newton, mesh, V->deg, F, live[k],
                               scratch + P.mat[tag], st)))
        return rc;
      continue;
    }
    const bool mat = kind == FLOW_BLOCK_MATRIX;
    if ((rc = launch_block_program(mat ? Element::matrix : Element::vector, mesh, V->deg,
                                   F, live[k], (mat ? mseen[tag]++ : vseen[tag]++) == 0,
                                   scratch + (mat ? P.mat[tag] : P.vec[tag]), spare,
                                   mat ? mplane : vplane, st)))
      return rc;
  }
  hipLaunchKernelGGL(
      block_newton_gather_kernel,
      dim3(grid_for(static_cast<long long>(V->nnz) + V->n, kBlock, 1 << 20)), dim3(kBlock),
      0, st, V->nnz, V->n, V->cptr, V->csrc, V->vptr, V->vsrc, scratch, P, plane_stride,
      vals, b);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

}  // namespace flow

using namespace flow;

extern "C" int flow_form_functional(const flow_mesh* mesh, const flow_form* form,
                                    double* scratch, double* work,
                                    double* result_host, void* stream) {
  int rc = check_form_mesh(mesh);
  if (rc) return rc;
  if ((rc = check_form(form))) return rc;
  FLOW_REQUIRE(form->nout == 1, "a functional has one output");
  FLOW_REQUIRE(scratch && work && result_host, "pointers");
  hipStream_t st = as_stream(stream);
  const int cb = mesh->c1 > 0 ? mesh->c0 : 0;
  const int ce = mesh->c1 > 0 ? mesh->c1 : mesh->nc;
  if ((rc = launch_cells(mesh, form, 0, cb, ce, scratch, st))) return rc;
  const int nparts = grid_for(ce - cb, kBlock, kRedBlocks);
  hipLaunchKernelGGL(form_sum_kernel, dim3(nparts), dim3(kBlock), 0, st, cb, ce,
                     scratch, work);
  FLOW_CHECK_LAUNCH();
  return sum_partials_host(work, nparts, result_host, st);
}

extern "C" int flow_form_cell_values(const flow_mesh* mesh, const flow_form* form,
                                     double* out, void* stream) {
  int rc = check_form_mesh(mesh);
  if (rc) return rc;
  FLOW_REQUIRE(mesh->c1 == 0, "per-cell integrals on strips");
  if ((rc = check_form(form))) return rc;
  FLOW_REQUIRE(form->nout == 1, "a functional has one output");
  FLOW_REQUIRE(out, "out pointer");
  return launch_cells(mesh, form, 0, 0, mesh->nc, out, as_stream(stream));
}

extern "C" int flow_form_load_vector(const flow_mesh* mesh, const flow_space* V,
                                     const flow_form* form, double* scratch,
                                     double* b, void* stream) {
  int rc = check_form_mesh(mesh);
  if (rc) return rc;
  if ((rc = check_form(form))) return rc;
  FLOW_REQUIRE(V && (V->deg == 1 || V->deg == 2) && V->n > 0 && V->vptr && V->vsrc,
               "space");
  FLOW_REQUIRE(V->r1 == 0 || (0 <= V->r0 && V->r0 < V->r1 && V->r1 <= V->n),
               "space row range");
  FLOW_REQUIRE(scratch && b, "pointers");
  hipStream_t st = as_stream(stream);
  const int cb = mesh->c1 > 0 ? mesh->c0 : 0;
  const int ce = mesh->c1 > 0 ? mesh->c1 : mesh->nc;
  if ((rc = launch_cells(mesh, form, V->deg, cb, ce, scratch, st))) return rc;
  const int nl = V->deg == 1 ? 3 : 6;
  return gather(V->n, form->nout, V->vptr, V->vsrc, scratch,
                static_cast<size_t>(nl) * mesh->nc, b, st, 0, V->r0, V->r1);
}

extern "C" int flow_form_facet_functional(const flow_mesh* mesh, const flow_form* form,
                                          int nfacets, const int* facet_cell,
                                          const int* facet_local, double* scratch,
                                          double* work, double* result_host,
                                          void* stream) {
  int rc = check_form_mesh(mesh);
  if (rc) return rc;
  FLOW_REQUIRE(mesh->c1 == 0, "facet integrals on strips");
  if ((rc = check_form(form, 3, true))) return rc;
  FLOW_REQUIRE(form->nout == 1, "a functional has one output");
  FLOW_REQUIRE(nfacets >= 0 && result_host, "facet count / result pointer");
  if (nfacets == 0) {
    *result_host = 0.0;
    return FLOW_OK;
  }
  FLOW_REQUIRE(facet_cell && facet_local, "facet lists");
  FLOW_REQUIRE(scratch && work, "pointers");
  hipStream_t st = as_stream(stream);
  if ((rc = launch_facets(mesh, form, nfacets, facet_cell, facet_local, scratch, st)))
    return rc;
  const int nparts = grid_for(nfacets, kBlock, kRedBlocks);
  hipLaunchKernelGGL(form_sum_kernel, dim3(nparts), dim3(kBlock), 0, st, 0, nfacets,
                     scratch, work);
  FLOW_CHECK_LAUNCH();
  return sum_partials_host(work, nparts, result_host, st);
}

extern "C" int flow_form_facet_values(const flow_mesh* mesh, const flow_form* form,
                                      int nfacets, const int* facet_cell,
                                      const int* facet_local, const int* facet_dest,
                                      const int* facet_flip, double* values,
                                      double* integrals, void* stream) {
  int rc = check_form_mesh(mesh);
  if (rc) return rc;
  FLOW_REQUIRE(mesh->c1 == 0, "wall distributions on strips");
  if ((rc = check_form(form, 3, true))) return rc;
  FLOW_REQUIRE(nfacets >= 0, "facet count");
  if (nfacets == 0) return FLOW_OK;
  FLOW_REQUIRE(static_cast<long long>(nfacets) * form->nq < (1LL << 31) - kBlock,
               "facet count (samples)");
  FLOW_REQUIRE(facet_cell && facet_local && facet_dest && facet_flip, "facet lists");
  FLOW_REQUIRE(values, "values pointer");
  return launch_facet_values(mesh, form, nfacets, facet_cell, facet_local, facet_dest,
                             facet_flip, values, integrals, as_stream(stream));
}

// what the two interior-facet entry points ask; *minus_slots as check_form
static int check_interior_facets(const flow_mesh* mesh, const flow_form* form,
                                 int nfacets, int* minus_slots) {
  int rc = check_form_mesh(mesh);
  if (rc) return rc;
  FLOW_REQUIRE(mesh->c1 == 0, "interior-facet integrals on strips");
  if ((rc = check_form(form, 3, true, false, 0, nullptr, minus_slots))) return rc;
  FLOW_REQUIRE(form->nout == 1, "an interior-facet integrand has one output");
  FLOW_REQUIRE(nfacets >= 0, "facet count");
  return FLOW_OK;
}

extern "C" int flow_form_interior_facet_functional(
    const flow_mesh* mesh, const flow_form* form, int nfacets, const int* facet_plus,
    const int* local_plus, const int* facet_other, double* scratch, double* work,
    double* result_host, void* stream) {
  int minus_slots = 0;
  int rc = check_interior_facets(mesh, form, nfacets, &minus_slots);
  if (rc) return rc;
  FLOW_REQUIRE(result_host, "result pointer");
  if (nfacets == 0) {
    *result_host = 0.0;
    return FLOW_OK;
  }
  FLOW_REQUIRE(facet_plus && local_plus && facet_other, "facet lists");
  FLOW_REQUIRE(scratch && work, "pointers");
  hipStream_t st = as_stream(stream);
  if ((rc = launch_interior_facets(mesh, form, nfacets, facet_plus, local_plus,
                                   facet_other, minus_slots, scratch, st)))
    return rc;
  const int nparts = grid_for(nfacets, kBlock, kRedBlocks);
  hipLaunchKernelGGL(form_sum_kernel, dim3(nparts), dim3(kBlock), 0, st, 0, nfacets,
                     scratch, work);
  FLOW_CHECK_LAUNCH();
  return sum_partials_host(work, nparts, result_host, st);
}

extern "C" int flow_form_interior_facet_values(
    const flow_mesh* mesh, const flow_form* form, int nfacets, const int* facet_plus,
    const int* local_plus, const int* facet_other, double* out, void* stream) {
  int minus_slots = 0;
  const int rc = check_interior_facets(mesh, form, nfacets, &minus_slots);
  if (rc) return rc;
  if (nfacets == 0) return FLOW_OK;
  FLOW_REQUIRE(facet_plus && local_plus && facet_other, "facet lists");
  FLOW_REQUIRE(out, "out pointer");
  return launch_interior_facets(mesh, form, nfacets, facet_plus, local_plus, facet_other,
                                minus_slots, out, as_stream(stream));
}

extern "C" int flow_facet_cell_shares(const flow_mesh* mesh, int nfacets,
                                      const int* position, const double* values,
                                      double share, double* out, void* stream) {
  const int rc = check_form_mesh(mesh);
  if (rc) return rc;
  FLOW_REQUIRE(mesh->c1 == 0, "facet shares on strips");
  FLOW_REQUIRE(nfacets >= 0 && position && out && (nfacets == 0 || values),
               "facet count / pointers");
  hipLaunchKernelGGL(facet_cell_shares_kernel, dim3((mesh->nc + kBlock - 1) / kBlock),
                     dim3(kBlock), 0,
                     as_stream(stream), mesh->nc, nfacets, position, values, share, out);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

extern "C" int flow_profile_cumsum(int ncurves, const int* curve_facets, int nrows,
                                   int nfacets, const double* integrals, double* out,
                                   void* stream) {
  FLOW_REQUIRE(ncurves >= 0 && nrows >= 0 && nfacets >= 0, "counts");
  FLOW_REQUIRE(ncurves == 0 || nrows <= ((1 << 30) / FLOW_PROFILE_CURVES_PER_LAUNCH),
               "row count");
  FLOW_REQUIRE(curve_facets, "curve offsets");
  FLOW_REQUIRE(curve_facets[0] == 0 && curve_facets[ncurves] == nfacets,
               "curve offsets (first 0, last nfacets)");
  for (int c = 0; c < ncurves; ++c)
    FLOW_REQUIRE(curve_facets[c] <= curve_facets[c + 1], "curve offsets (sorted)");
  if (ncurves == 0 || nrows == 0 || nfacets == 0) return FLOW_OK;
  FLOW_REQUIRE(integrals && out, "pointers");
  hipStream_t st = as_stream(stream);
  for (int c0 = 0; c0 < ncurves; c0 += FLOW_PROFILE_CURVES_PER_LAUNCH) {
    const int n = ncurves - c0 < FLOW_PROFILE_CURVES_PER_LAUNCH
                      ? ncurves - c0 : FLOW_PROFILE_CURVES_PER_LAUNCH;
    ProfileCurves C;
    for (int k = 0; k <= FLOW_PROFILE_CURVES_PER_LAUNCH; ++k)
      C.off[k] = curve_facets[c0 + (k < n ? k : n)];
    hipLaunchKernelGGL(profile_cumsum_kernel, dim3((n * nrows + kBlock - 1) / kBlock),
                       dim3(kBlock), 0, st, n, C, nrows, nfacets, integrals, out);
    FLOW_CHECK_LAUNCH();
  }
  return FLOW_OK;
}

static int check_point_grid(const flow_point_grid* grid) {
  FLOW_REQUIRE(grid && grid->nx >= 1 && grid->ny >= 1 &&
                   static_cast<long long>(grid->nx) * grid->ny < (1LL << 31) - 1,
               "point grid size");
  FLOW_REQUIRE(grid->hx_inv > 0.0 && grid->hy_inv > 0.0 && std::isfinite(grid->hx_inv) &&
                   std::isfinite(grid->hy_inv) && std::isfinite(grid->x0) && std::isfinite(grid->y0),
               "point grid geometry");
  FLOW_REQUIRE(grid->start && grid->cells, "point grid arrays");
  return FLOW_OK;
}

extern "C" int flow_locate_points(const flow_mesh* mesh, const flow_point_grid* grid,
                                  int n, const double* xy, int* cell, double* bary,
                                  void* stream) {
  int rc = check_form_mesh(mesh);
  if (rc) return rc;
  if ((rc = check_point_grid(grid))) return rc;
  FLOW_REQUIRE(n >= 0, "point count");
  if (n == 0) return FLOW_OK;
  FLOW_REQUIRE(xy && cell && bary, "pointers");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(locate_points_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock),
                     0, st, mesh->nc, mesh->xy, *grid, n, xy, cell, bary);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

template <int DEG, int SCHEME>
static void launch_advect(const flow_mesh* mesh, const flow_point_grid* grid,
                          const flow_space* W, const double* u, const double* u_next,
                          int n, double* xy, int* cell, double* bary, double dt,
                          int steps, hipStream_t st) {
  const dim3 blocks((n + kBlock - 1) / kBlock);
  if (u_next)
    hipLaunchKernelGGL((advect_points_kernel<DEG, SCHEME, true>), blocks, dim3(kBlock),
                       0, st, mesh->nc, mesh->xy, *grid, W->cell_dofs, W->n, u, u_next,
                       n, xy, cell, bary, dt, steps);
  else
    hipLaunchKernelGGL((advect_points_kernel<DEG, SCHEME, false>), blocks, dim3(kBlock),
                       0, st, mesh->nc, mesh->xy, *grid, W->cell_dofs, W->n, u, u_next,
                       n, xy, cell, bary, dt, steps);
}

extern "C" int flow_advect_points(const flow_mesh* mesh, const flow_point_grid* grid,
                                  const flow_space* W, const double* u,
                                  const double* u_next, int n, double* xy, int* cell,
                                  double* bary, double dt, int steps, int scheme,
                                  void* stream) {
  int rc = check_form_mesh(mesh);
  if (rc) return rc;
  FLOW_REQUIRE(mesh->c1 == 0, "tracer particles on strips");
  if ((rc = check_point_grid(grid))) return rc;
  FLOW_REQUIRE(W && (W->deg == 1 || W->deg == 2) && W->n >= 1 && W->cell_dofs,
               "velocity space");
  FLOW_REQUIRE(u, "velocity");
  FLOW_REQUIRE(scheme == FLOW_ADVECT_EULER || scheme == FLOW_ADVECT_RK2 ||
                   scheme == FLOW_ADVECT_RK4,
               "scheme");
  FLOW_REQUIRE(steps >= 1, "substeps");
  FLOW_REQUIRE(std::isfinite(dt), "time step");
  FLOW_REQUIRE(n >= 0, "point count");
  if (n == 0) return FLOW_OK;
  FLOW_REQUIRE(xy && cell && bary, "pointers");
  hipStream_t st = as_stream(stream);
#define FLOW_ADVECT(DEG, SCHEME)                                                   \
  launch_advect<DEG, SCHEME>(mesh, grid, W, u, u_next, n, xy, cell, bary, dt, steps, st)
  if (W->deg == 1) {
    if (scheme == FLOW_ADVECT_EULER) FLOW_ADVECT(1, 1);
    else if (scheme == FLOW_ADVECT_RK2) FLOW_ADVECT(1, 2);
    else FLOW_ADVECT(1, 4);
  } else {
    if (scheme == FLOW_ADVECT_EULER) FLOW_ADVECT(2, 1);
    else if (scheme == FLOW_ADVECT_RK2) FLOW_ADVECT(2, 2);
    else FLOW_ADVECT(2, 4);
  }
#undef FLOW_ADVECT
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}

extern "C" int flow_form_points(const flow_mesh* mesh, const flow_form* form, int n,
                                const int* cell, const double* bary, double* out,
                                void* stream) {
  int rc = check_form_mesh(mesh);
  if (rc) return rc;
  FLOW_REQUIRE(mesh->c1 == 0, "point evaluation on strips");
  if ((rc = check_form(form, 1, false, true))) return rc;
  FLOW_REQUIRE(n >= 0, "point count");
  if (n == 0) return FLOW_OK;
  FLOW_REQUIRE(cell && bary && out, "pointers");
  return launch_points(mesh, form, n, cell, bary, out, as_stream(stream));
}

extern "C" int flow_form_matrix(const flow_mesh* mesh, const flow_space* V,
                                const flow_form* form, double* scratch,
                                double* vals, void* stream) {
  int rc = check_argument_space(mesh, V, true, false);
  if (rc) return rc;
  int live = 0;
  if ((rc = check_form(form, 1, false, false, FLOW_FORM_SLOTS, &live))) return rc;
  FLOW_REQUIRE(scratch && vals, "pointers");
  hipStream_t st = as_stream(stream);
  if ((rc = launch_element(Element::matrix, mesh, V->deg, form, live, scratch, st)))
    return rc;
  return gather(V->nnz, 1, V->cptr, V->csrc, scratch, 0, vals, st);
}

extern "C" int flow_form_vector(const flow_mesh* mesh, const flow_space* V,
                                const flow_form* form, double* scratch, double* b,
                                void* stream) {
  int rc = check_argument_space(mesh, V, false, true);
  if (rc) return rc;
  int live = 0;
  if ((rc = check_form(form, 1, false, false, 3, &live))) return rc;
  FLOW_REQUIRE(scratch && b, "pointers");
  hipStream_t st = as_stream(stream);
  if ((rc = launch_element(Element::vector, mesh, V->deg, form, live, scratch, st)))
    return rc;
  return gather(V->n, 1, V->vptr, V->vsrc, scratch,
                static_cast<size_t>(V->deg == 1 ? 3 : 6) * mesh->nc, b, st);
}

extern "C" int flow_form_newton(const flow_mesh* mesh, const flow_space* V,
                                const flow_form* form, double* scratch, double* vals,
                                double* b, void* stream) {
  int rc = check_argument_space(mesh, V, true, true);
  if (rc) return rc;
  int live = 0;
  if ((rc = check_form(form, 1, false, false, FLOW_FORM_NEWTON_SLOTS, &live))) return rc;
  FLOW_REQUIRE(scratch && vals && b, "pointers");
  hipStream_t st = as_stream(stream);
  if ((rc = launch_element(Element::newton, mesh, V->deg, form, live, scratch, st)))
    return rc;
  const int nl = V->deg == 1 ? 3 : 6;
  if ((rc = gather(V->nnz, 1, V->cptr, V->csrc, scratch, 0, vals, st))) return rc;
  return gather(V->n, 1, V->vptr, V->vsrc,
                scratch + static_cast<size_t>(nl) * nl * mesh->nc,
                static_cast<size_t>(nl) * mesh->nc, b, st);
}

extern "C" int flow_form_facet_matrix(const flow_mesh* mesh, const flow_space* V,
                                      const flow_form* form, int nfacets,
                                      const int* facet_cell, const int* facet_local,
                                      int ntargets, const int* map_targets,
                                      const int* map_ptr, const int* map_src,
                                      double* scratch, double* vals, void* stream) {
  return facet_arguments<2>(mesh, V, form, nfacets, facet_cell, facet_local, ntargets,
                            map_targets, map_ptr, map_src, scratch, vals, stream);
}

extern "C" int flow_form_facet_vector(const flow_mesh* mesh, const flow_space* V,
                                      const flow_form* form, int nfacets,
                                      const int* facet_cell, const int* facet_local,
                                      int ntargets, const int* map_targets,
                                      const int* map_ptr, const int* map_src,
                                      double* scratch, double* b, void* stream) {
  return facet_arguments<1>(mesh, V, form, nfacets, facet_cell, facet_local, ntargets,
                            map_targets, map_ptr, map_src, scratch, b, stream);
}

extern "C" int flow_form_cells_functional(const flow_mesh* mesh, const flow_form* form,
                                          int ncells, const int* cells, double* scratch,
                                          double* work, double* result_host,
                                          void* stream) {
  int rc = check_cell_list(mesh, form, ncells);
  if (rc) return rc;
  FLOW_REQUIRE(result_host, "result pointer");
  if (ncells == 0) {
    *result_host = 0.0;
    return FLOW_OK;
  }
  FLOW_REQUIRE(cells, "cell list");
  FLOW_REQUIRE(scratch && work, "pointers");
  hipStream_t st = as_stream(stream);
  if ((rc = launch_cell_list<false>(mesh, form, ncells, cells, scratch, st))) return rc;
  const int nparts = grid_for(ncells, kBlock, kRedBlocks);
  hipLaunchKernelGGL(form_sum_kernel, dim3(nparts), dim3(kBlock), 0, st, 0, ncells,
                     scratch, work);
  FLOW_CHECK_LAUNCH();
  return sum_partials_host(work, nparts, result_host, st);
}

extern "C" int flow_form_cells_values(const flow_mesh* mesh, const flow_form* form,
                                      int ncells, const int* cells, double* out,
                                      void* stream) {
  const int rc = check_cell_list(mesh, form, ncells);
  if (rc) return rc;
  if (ncells == 0) return FLOW_OK;
  FLOW_REQUIRE(cells, "cell list");
  FLOW_REQUIRE(out, "out pointer");
  return launch_cell_list<true>(mesh, form, ncells, cells, out, as_stream(stream));
}

extern "C" int flow_form_cells_matrix(const flow_mesh* mesh, const flow_space* V,
                                      const flow_form* form, int ncells, const int* cells,
                                      int ntargets, const int* map_targets,
                                      const int* map_ptr, const int* map_src,
                                      double* scratch, double* vals, void* stream) {
  return cells_arguments<2>(mesh, V, form, ncells, cells, ntargets, map_targets, map_ptr,
                            map_src, scratch, vals, stream);
}

extern "C" int flow_form_cells_vector(const flow_mesh* mesh, const flow_space* V,
                                      const flow_form* form, int ncells, const int* cells,
                                      int ntargets, const int* map_targets,
                                      const int* map_ptr, const int* map_src,
                                      double* scratch, double* b, void* stream) {
  return cells_arguments<1>(mesh, V, form, ncells, cells, ntargets, map_targets, map_ptr,
                            map_src, scratch, b, stream);
}

extern "C" int flow_form_block_matrix(const flow_mesh* mesh, const flow_space* V,
                                      int nprog, const flow_form* forms,
                                      const int* blocks, double* scratch, double* vals,
                                      size_t plane_stride, void* stream) {
  return block_arguments<2>(mesh, V, nprog, forms, blocks, scratch, vals, plane_stride,
                            stream);
}

extern "C" int flow_form_block_vector(const flow_mesh* mesh, const flow_space* V,
                                      int nprog, const flow_form* forms,
                                      const int* blocks, double* scratch, double* b,
                                      void* stream) {
  return block_arguments<1>(mesh, V, nprog, forms, blocks, scratch, b,
                            V ? static_cast<size_t>(V->n) : 0, stream);
}

extern "C" int flow_form_block_newton(const flow_mesh* mesh, const flow_space* V,
                                      int nprog, const flow_form* forms, const int* kinds,
                                      const int* tags, double* scratch, size_t nscratch,
                                      double* vals, size_t plane_stride, double* b,
                                      void* stream) {
  return block_newton(mesh, V, nprog, forms, kinds, tags, scratch, nscratch, vals,
                      plane_stride, b, stream);
}

extern "C" int flow_form_rect_matrix(const flow_mesh* mesh, const flow_space* V_test,
                                     const flow_space* V_trial, const flow_form* form,
                                     double* scratch, double* vals, const int* cptr,
                                     const int* csrc, int nnz, void* stream) {
  return rect_matrix(mesh, V_test, V_trial, form, scratch, vals, cptr, csrc, nnz, stream);
}

extern "C" int flow_form_rect_facet_matrix(
    const flow_mesh* mesh, const flow_space* V_test, const flow_space* V_trial,
    const flow_form* form, int nfacets, const int* facet_cell, const int* facet_local,
    int ntargets, const int* map_targets, const int* map_ptr, const int* map_src,
    double* scratch, double* vals, int nnz, void* stream) {
  return rect_list<true>(mesh, V_test, V_trial, form, nfacets, facet_cell, facet_local,
                         ntargets, map_targets, map_ptr, map_src, scratch, vals, nnz,
                         stream);
}

extern "C" int flow_form_rect_cells_matrix(
    const flow_mesh* mesh, const flow_space* V_test, const flow_space* V_trial,
    const flow_form* form, int ncells, const int* cells, int ntargets,
    const int* map_targets, const int* map_ptr, const int* map_src, double* scratch,
    double* vals, int nnz, void* stream) {
  return rect_list<false>(mesh, V_test, V_trial, form, ncells, cells, nullptr, ntargets,
                          map_targets, map_ptr, map_src, scratch, vals, nnz, stream);
}

extern "C" int flow_bc_rect_mask(const int* rowptr, const int* cols, int n_rows,
                                 double* vals, const unsigned char* row_isbc,
                                 const unsigned char* col_isbc, void* stream) {
  FLOW_REQUIRE(n_rows > 0, "row count");
  FLOW_REQUIRE(rowptr && cols && vals && row_isbc && col_isbc, "pointers");
  hipLaunchKernelGGL(bc_rect_mask_kernel, dim3((n_rows + kBlock - 1) / kBlock),
                     dim3(kBlock), 0, as_stream(stream), n_rows, rowptr, cols, row_isbc,
                     col_isbc, vals);
  FLOW_CHECK_LAUNCH();
  return FLOW_OK;
}
