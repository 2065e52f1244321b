/*
 * gaast_expr.h -- host-side mirror of gaast's phases 1-3 for hosts that are not Rust.
 *
 * A Rust host keeps the reference's own `Expr` / `specialize` (src/ast/expr.rs,
 * src/ast/specialize.rs) and only needs gaast_hip.h.  This header gives C, C++ and Python
 * hosts the same operator surface (same names, argument meaning and failure behaviour) so
 * that programs for gaast_hip_program_create() can be built and tests can read like the
 * reference's own.  It is host-only bookkeeping: no component value is touched here and no
 * GPU is needed.
 *
 * Every function cites the reference item it mirrors.  Failures that are panics upstream
 * return NULL / a non-zero status and leave a message in gaast_expr_last_error().
 */
#ifndef GAAST_EXPR_H
#define GAAST_EXPR_H

#include <stddef.h>
#include <stdint.h>

#include "gaast_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gaast_expr_s *gaast_expr_t;        /* Expr<'a, T>        src/ast/expr.rs:29-44 */
typedef struct gaast_spec_s *gaast_spec_t;        /* SpecializedAst<T>  src/ast/specialize.rs:10-13 */

/* grades_to_produce closure of Expr::product (expr.rs:123-127): returns the grade mask wanted
 * out of the product of a k1-vector and a k2-vector. */
typedef uint64_t (*gaast_select_fn)(int64_t k1, int64_t k2, void *user);

const char *gaast_expr_last_error(void);

/* ---- GradeSet algebra on 64-bit masks (src/grade_set.rs) -------------------------------- */
uint64_t gaast_gs_single(int64_t k);                      /* grade_set.rs:65-71 (negative -> empty) */
uint64_t gaast_gs_range(int x, int y);                    /* grade_set.rs:74-80 */
uint64_t gaast_gs_mul(uint64_t a, uint64_t b);            /* grade_set.rs:305-327 (no dimension cap) */
/* the five closures of expr.rs:180-197.  GAAST_PROD_REGRESSIVE produces grade k1 + k2 - n, which depends on the dimension that
 * neither this function nor gaast_gs_parts_contributing_to_product takes: both answer "nothing" (0) for that kind; specialise an
 * expression to see its grades. */
uint64_t gaast_gs_select(int kind, int64_t k1, int64_t k2);
/* grade_set.rs:239-252 */
void gaast_gs_parts_contributing_to_product(uint64_t self, int kind, uint64_t left, uint64_t right,
                                            uint64_t *out_left, uint64_t *out_right);

/* ---- Algebra (src/algebra.rs) -------------------------------------------------------------- */
uint64_t gaast_n_choose_k(uint64_t n, uint64_t k);                       /* algebra.rs:252-254 */
uint64_t gaast_component_to_blade(int n, int grade, uint64_t index);     /* algebra.rs:31-37 */
uint64_t gaast_blade_to_component(int n, uint64_t blade, int *grade);    /* algebra.rs:41-45 */
/* ortho_basis_blades_gp, algebra.rs:73-83: returns the coefficient, *res = b1 ^ b2 */
double gaast_blades_gp(int n, const double *metric_diag, uint64_t b1, uint64_t b2, uint64_t *res);
/* Non-diagonal metrics: the reference's MetricAlgebra::base_vec_dot(i, j) as a full Gram matrix (algebra.rs:57-66, whose
 * TODO is its diagonalisation, algebra.rs:68-83).  gram: row-major n x n, finite and exactly symmetric, 1 <= n <= GAAST_MAX_DIM
 * (else GAAST_ERR_INVALID_ARGUMENT).  G = Q diag(L) Q^T by cyclic Jacobi in double: diag_out[j] = L_j, basis_out[i*n + j] = Q_ij,
 * coordinate i of the orthogonal basis vector f_j = sum_i Q_ij e_i.  Deterministic (same input, same bits): every column's
 * largest-magnitude entry is positive; |L_j| <= 64 eps max|L| becomes exactly 0 (a degenerate metric stays degenerate).  An
 * exactly diagonal G gives Q = I and L = diag(G) bit for bit, in the original order (no sorting). */
int gaast_metric_diagonalize(int n, const double *gram, double *diag_out, double *basis_out);
/* k-th compound of an n x n matrix (row-major): out is C(n,k) x C(n,k), row-major, out[I*C(n,k) + J] = det m[rows of blade I,
 * columns of blade J], I and J in the component order of grade k (gaast_component_to_blade).  C_k(M) is the outermorphism of M
 * on grade k: the coordinates of M e_J = (M e_j1) ^ ... ^ (M e_jk) are column J. */
int gaast_compound_matrix(int n, const double *m, int k, double *out);
/* Reverse mode of gaast_compound_matrix with respect to the matrix.  w: C(n,k) x C(n,k), row-major, w[I*C(n,k) + J] = dL/dC_k(M)[I][J].
 * ADDS grade k's contribution to dmatrix (n x n, row-major; the caller zeroes it and calls once per grade), in double:
 *   dmatrix[i*n + j] += sum over blades I containing i and J containing j of (-1)^(p_I(i) + p_J(j)) C_{k-1}(M)[I \ i][J \ j] w[I][J],
 * p the 0-based position of the vector in the ascending blade: the cofactor expansion of each k x k minor.  C_0 = (1), so k = 1
 * adds w itself; k = 0 adds nothing (C_0 does not depend on M).  Terms are added in the order I, J, i, j ascending.  The device
 * contraction of gaast_hip_linmap_matrix_vjp (gaast_hip.h) is built from the same term list. */
int gaast_compound_matrix_vjp(int n, int k, const double *matrix, const double *w, double *dmatrix);

/* ---- Expr construction (phase 1) -------------------------------------------------------------- */
gaast_expr_t gaast_expr_retain(gaast_expr_t e);  /* Expr::clone, expr.rs:47-53: same node identity */
void gaast_expr_release(gaast_expr_t e);
/* mv(x), expr.rs:162-164, for an input that is bound at evaluation time: `slot` names it,
 * grade_mask / storage_dim are what T::grade_set() and its slice lengths would report. */
gaast_expr_t gaast_expr_input(int slot, uint64_t grade_mask, int storage_dim);
/* mv(x) for a value fixed at build time (shared by all batch items); row = grades ascending. */
gaast_expr_t gaast_expr_const(uint64_t grade_mask, int storage_dim, const double *row, size_t row_len);
gaast_expr_t gaast_expr_from_f64(double x);                       /* expr.rs:231-240 */
gaast_expr_t gaast_expr_basis_vector(int dim, int i);             /* expr.rs:148-157 */
gaast_expr_t gaast_expr_product(gaast_expr_t l, gaast_expr_t r, int kind); /* expr.rs:166-197 */
gaast_expr_t gaast_expr_product_custom(gaast_expr_t l, gaast_expr_t r, gaast_select_fn f,
                                       void *user);                /* expr.rs:123-144 */
gaast_expr_t gaast_expr_add(gaast_expr_t l, gaast_expr_t r);      /* expr.rs:200-210 */
gaast_expr_t gaast_expr_neg(gaast_expr_t e);                      /* expr.rs:213-221 */
gaast_expr_t gaast_expr_sub(gaast_expr_t l, gaast_expr_t r);      /* expr.rs:224-229 */
gaast_expr_t gaast_expr_div_scalar(gaast_expr_t e, double s);     /* expr.rs:265-270 */
gaast_expr_t gaast_expr_rev(gaast_expr_t e);                      /* expr.rs:292 */
gaast_expr_t gaast_expr_ginvol(gaast_expr_t e);                   /* expr.rs:293 */
gaast_expr_t gaast_expr_exp(gaast_expr_t e);                      /* expr.rs:294 */
gaast_expr_t gaast_expr_log(gaast_expr_t e);                      /* expr.rs:295 */
gaast_expr_t gaast_expr_pow(gaast_expr_t e, gaast_expr_t p);      /* expr.rs:300-302 */
gaast_expr_t gaast_expr_sqrt(gaast_expr_t e);                     /* expr.rs:305-319 */
gaast_expr_t gaast_expr_g(gaast_expr_t e, int64_t k);             /* expr.rs:322-324 */
gaast_expr_t gaast_expr_gselect_mask(gaast_expr_t e, uint64_t wanted); /* expr.rs:327-335 */
gaast_expr_t gaast_expr_conj(gaast_expr_t e);                     /* expr.rs:338-340 */
gaast_expr_t gaast_expr_scal(gaast_expr_t e, gaast_expr_t rhs);   /* expr.rs:343-345 */
gaast_expr_t gaast_expr_norm_sq(gaast_expr_t e);                  /* expr.rs:348-350 */
gaast_expr_t gaast_expr_sinv(gaast_expr_t e);                     /* expr.rs:353-358 */
gaast_expr_t gaast_expr_vinv(gaast_expr_t e);                     /* expr.rs:363-371 */
/* no reference counterpart: the right / left complement (GAAST_OP_DUAL / GAAST_OP_UNDUAL, gaast_hip.h); a v b is
 * gaast_expr_product with GAAST_PROD_REGRESSIVE */
gaast_expr_t gaast_expr_dual(gaast_expr_t e);
gaast_expr_t gaast_expr_undual(gaast_expr_t e);
/* no reference counterpart: the general multivector inverse (GAAST_OP_INV, gaast_hip.h), the Y with e Y = 1 whether or not e is a
 * versor; the result holds the even grades for an even operand, every grade otherwise; a scalar operand is gaast_expr_sinv */
gaast_expr_t gaast_expr_inv(gaast_expr_t e);
/* no reference counterpart: the general multivector exponential (GAAST_OP_GEXP, gaast_hip.h), sum_k e^k / k! for any multivector
 * by scaling and squaring, where gaast_expr_exp is a closed form for k-vectors whose square is a scalar; grades as gaast_expr_inv */
gaast_expr_t gaast_expr_gexp(gaast_expr_t e);
/* no reference counterpart: the general multivector square root (GAAST_OP_GSQRT, gaast_hip.h), the principal X with X X = e for any
 * multivector that has one, where gaast_expr_sqrt is a closed form for k-vectors whose square is a scalar; grades as
 * gaast_expr_inv; a scalar operand is the scalar square root (GAAST_OP_SSQRT) */
gaast_expr_t gaast_expr_gsqrt(gaast_expr_t e);
/* no reference counterpart: the general multivector logarithm (GAAST_OP_GLOG, gaast_hip.h), the principal Y with gexp(Y) = e for any
 * multivector that has one, by inverse scaling and squaring, where gaast_expr_log is a closed form for k-vectors whose square is a
 * scalar; grades as gaast_expr_inv; no scalar lowering (a scalar operand is evaluated over the even blades) */
gaast_expr_t gaast_expr_glog(gaast_expr_t e);

/* ---- reify + specialize (phases 2-3) ---------------------------------------------------------- */
/* Expr::specialize(&alg), specialize.rs:36-50, with alg = the diagonal metric `metric_diag[n]`
 * ([f64; D], algebra.rs:148-165; all ones = OrthoEuclidN(n), algebra.rs:173-192).
 * materialize_limit: PRODUCT nodes whose comp-mul list would exceed this many entries keep a
 * compact descriptor instead of the explicit list (0 = always explicit). */
gaast_spec_t gaast_expr_specialize(gaast_expr_t e, int n, const double *metric_diag,
                                   uint64_t materialize_limit);
void gaast_spec_free(gaast_spec_t s);

/* public read API of SpecializedAst / GradedNode (specialize.rs:17-24, base_types.rs:124-146);
 * nodes are numbered in post-order, the root is the last one. */
int gaast_spec_num_nodes(gaast_spec_t s);
int gaast_spec_root(gaast_spec_t s);
typedef struct gaast_spec_node_info {
    int32_t opcode;           /* gaast_opcode */
    int32_t child0, child1;
    uint64_t maximal_grade_mask;
    uint64_t minimal_grade_mask;
    int32_t vec_space_dim;
    int32_t num_uses;
    int32_t input_slot;       /* OP_INPUT: slot, or -(1+const index) for embedded constants */
    int32_t product_kind;
    uint64_t n_comp_muls;     /* length the explicit list has / would have */
} gaast_spec_node_info;
int gaast_spec_node(gaast_spec_t s, int idx, gaast_spec_node_info *out);
/* Product.individual_comp_muls (NULL when the node kept a compact descriptor) */
const gaast_comp_mul *gaast_spec_comp_muls(gaast_spec_t s, int idx);

/* The flat program for gaast_hip_program_create(); pointers stay valid until gaast_spec_free.
 * Embedded constants are appended after the caller's input slots. */
int gaast_spec_program_desc(gaast_spec_t s, int dtype, uint32_t flags, gaast_program_desc *out);
/* ---- program wire format ------------------------------------------------------
 * The reference's SpecializedAst cannot be stored (closures and pointer ids, base_types.rs:60-64,
 * 92-96); the flat program can.  Layout (little endian): "GAASTPRG", u32 version = 1, then the
 * fields of gaast_program_desc in order, every array length-prefixed; comp-mul lists as 32-byte
 * gaast_comp_mul records.  gaast_program_serialize returns the number of bytes needed / written
 * (call with buf = NULL to size); gaast_program_deserialize returns a handle that owns the
 * decoded arrays, or NULL on a malformed image. */
typedef struct gaast_program_image_s *gaast_program_image_t;
size_t gaast_program_serialize(const gaast_program_desc *desc, void *buf, size_t cap);
gaast_program_image_t gaast_program_deserialize(const void *buf, size_t len);
const gaast_program_desc *gaast_program_image_desc(gaast_program_image_t img);
void gaast_program_image_free(gaast_program_image_t img);

/* ---- reverse mode ---------------------------------------------------------------------------------
 * The vector-Jacobian product of a flat program with respect to input `wrt_slot`, as a new flat program (read it with
 * gaast_program_image_desc, free it with gaast_program_image_free).  It differentiates the program as eval.rs evaluates it,
 * including the in-place order of a node's operations (a Negation / Reverse / GradeInvolution / scalar op acts on everything
 * accumulated so far into the buffer of the product operand or root that contains it).
 * Inputs: slots 0 .. n_inputs - 1 are desc's, unchanged (const ones included); slot n_inputs is the cotangent (grade mask = the
 * root's minimal mask, storage dimension n, batched); a const scalar 1 may follow at slot n_inputs + 1 (used by sign changes and
 * projections of a cotangent).  Output: the gradient rows in input wrt_slot's layout (its grade mask and storage dimension), zero
 * when the input does not reach the root.  An explicit list gets its explicit transposed list; a compact product, and a geometric
 * product (product_kind GAAST_PROD_GEOMETRIC) at n >= 6 whatever its form, a compact GAAST_PROD_ADJ_LEFT / GAAST_PROD_ADJ_RIGHT node,
 * which the dense kernels evaluate where they take the forward product.  The adjoint program inherits desc->flags.
 * A GAAST_OP_DUAL / GAAST_OP_UNDUAL node gives its operand the OTHER complement of its buffer's cotangent restricted to the node's
 * grades (the transpose of a signed permutation is its inverse); GAAST_PROD_REGRESSIVE differentiates like kinds 1-4, and an explicit
 * transposed list of it keeps product_kind = GAAST_PROD_REGRESSIVE (the orientation sign of a Gram basis applies to it too).
 * A GAAST_OP_INV node Y = inv(A) gives A the cotangent -ADJ_RIGHT(ADJ_LEFT(g, Y), Y) (geometric adjoint products and a
 * GAAST_OP_NEG; Y is one more GAAST_OP_INV node over the forward operand, producing every grade of its blade set).
 * A GAAST_OP_GEXP node gives its operand one GAAST_OP_GEXP_ADJ node over (the buffer's cotangent restricted to the node's grades,
 * the forward operand); no flag is needed.  A GAAST_OP_GSQRT node likewise gives its operand one GAAST_OP_GSQRT_ADJ node,
 * a GAAST_OP_GLOG node one GAAST_OP_GLOG_ADJ node.
 * A program specialised for the orthogonal basis of a Gram metric differentiates like any other: its VJP program is created with the
 * same basis (gaast_hip_program_create_vjp_in_basis, gaast_hip.h), the cotangent being one more batched input.
 * Closure: desc may itself be a program this function returned, to any depth (second-order reverse mode, Hessian-vector products,
 * forward mode as the VJP of a VJP with respect to its cotangent).  Every non-const slot of such a program is a valid wrt_slot, its
 * cotangent slot included; the const 1 of the program differentiated stays where it is, the new cotangent is appended at its
 * n_inputs and a const 1 of the new program after that.  The image returned for a forward program is not affected by any of this.
 * A compact adjoint product (product_kind = base + GAAST_PROD_ADJ_LEFT or base + GAAST_PROD_ADJ_RIGHT, base = 0..5; any other kind
 * above 7 is GAAST_ERR_INVALID_PROGRAM) is an ordinary product of two operand buffers.  With T(g, a, b) = <g, a o b> the trilinear
 * form of the forward kind and h the cotangent of the node, restricted to the node's grades:
 *     node P                                    operand      its cotangent
 *     ADJ_LEFT + base, children (g, b),         child0 = g   forward base, children (h, b), mask of g
 *       mask of a                               child1 = b   ADJ_RIGHT + base, children (g, h), mask of b
 *     ADJ_RIGHT + base, children (g, a),        child0 = g   forward base, children (a, h), mask of g  (note the order)
 *       mask of b                               child1 = a   ADJ_LEFT + base, children (g, h), mask of a
 * so a product differentiated any number of times stays within {base, ADJ_LEFT + base, ADJ_RIGHT + base} of one kind, n_comp_muls
 * counted from the three grade sets as at first order; GAAST_PROD_REGRESSIVE keeps its kind in every form (a Gram basis applies its
 * orientation sign once per node), and an explicit list stays explicit.  GAAST_OP_INV needs nothing else: its adjoint is a
 * GAAST_OP_NEG, one more GAAST_OP_INV and two geometric adjoint products.
 * The adjoint op nodes GAAST_OP_EXP_ADJ, GAAST_OP_LOG_ADJ, GAAST_OP_GEXP_ADJ, GAAST_OP_GSQRT_ADJ and GAAST_OP_GLOG_ADJ are valid nodes
 * with two children; off the path to wrt_slot they are carried along untouched.  So are GAAST_OP_GEXP_JVP (two children) and
 * GAAST_OP_GEXP_ADJ2 / GAAST_OP_GLOG_ADJ2 (three: the third, the forward operand, is the node index in input_slot, which the renumbering of the image
 * follows like child0 and child1).
 * Second order through the general exponential (OPT-IN: GAAST_FLAG_GEXP_GRAD2 in desc->flags; only this function reads the flag, the
 * image inherits it).  With k the cotangent of the node's buffer restricted to the node's grades:
 *     node on the path          through   its operand's cotangent
 *     GEXP_ADJ(g, A)            g         GEXP_JVP(k, A), mask of g
 *     GEXP_ADJ(g, A)            A         GEXP_ADJ2(g, k, A), mask of A
 *     GEXP_JVP(t, A)            t         GEXP_ADJ(k, A), mask of t
 *     GEXP_JVP(t, A)            A         GEXP_ADJ2(k, t, A), mask of A
 *     GEXP_ADJ2                 any       GAAST_ERR_UNIMPLEMENTED ("third-order reverse mode through GAAST_OP_GEXP_ADJ2 ...")
 * so the family {GEXP_ADJ, GEXP_JVP, GEXP_ADJ2} is closed up to second order: Hessian-vector products, forward mode (the VJP of the
 * VJP with respect to its cotangent holds GEXP_JVP and never reads the first cotangent) and the transpose of forward mode all work
 * through gexp.  Without the flag GEXP_ADJ on the path is refused as before and GEXP_JVP in the same words; a forward image is the
 * same with and without the flag, a first-order image differs in its flags word only.
 * Forward mode through the general square root and logarithm, any order through the root (OPT-IN: GAAST_FLAG_GSQRT_GLOG_JVP, read and
 * inherited like GAAST_FLAG_GEXP_GRAD2; GAAST_OP_GSQRT_JVP and GAAST_OP_GLOG_JVP are two-child nodes like GAAST_OP_GEXP_JVP, no third
 * child).  Both adjoint nodes are linear in their cotangent, so its derivative is the transposed map, the tangent of the forward at
 * the same operand.  With k as above, S = L_X + R_X at the root X of A, w and u on every grade of the blade set:
 *     node on the path          through   its operand's cotangent
 *     GSQRT_ADJ(g, A)           g         GSQRT_JVP(k, A), mask of g
 *     GSQRT_ADJ(g, A)           A         -GSQRT_ADJ(ADJ_LEFT(w, u) + ADJ_RIGHT(w, u), A), w = GSQRT_ADJ(g, A), u = GSQRT_JVP(k, A)
 *     GSQRT_JVP(h, A)           h         GSQRT_ADJ(k, A), mask of h
 *     GSQRT_JVP(h, A)           A         the same expression with w = GSQRT_ADJ(k, A), u = GSQRT_JVP(h, A)
 *     GLOG_ADJ(g, A)            g         GLOG_JVP(k, A), mask of g
 *     GLOG_JVP(h, A)            h         GLOG_ADJ(k, A), mask of h
 *     GLOG_ADJ / GLOG_JVP       A         GAAST_ERR_UNIMPLEMENTED ("reverse mode through GAAST_OP_GLOG_ADJ with respect to its operand ...")
 *   and with GAAST_FLAG_GLOG_GRAD2 beside the flag (alone it changes nothing), in the place of the last line:
 *     GLOG_ADJ(g, A)            A         GLOG_ADJ2(g, k, A), mask of A
 *     GLOG_JVP(h, A)            A         GLOG_ADJ2(k, h, A), mask of A
 *     GLOG_ADJ2                 any       GAAST_ERR_UNIMPLEMENTED ("third-order reverse mode through GAAST_OP_GLOG_ADJ2 ...")
 * The operand rule is the gradient in A of <g, S^-1 h>: d(S^-1) = -S^-1 (L_dX + R_dX) S^-1 and dX = S^-1 dA.  ADJ_LEFT / ADJ_RIGHT are
 * compact geometric adjoint products, the sign one GAAST_OP_NEG on k (the innermost child, as for GAAST_OP_INV); every node is one
 * the function emits elsewhere, so the family of gsqrt is closed at EVERY order.  A GLOG node is refused only when its operand
 * depends on wrt_slot; reached through child0 alone (forward mode) it is accepted.  Without the flag all four nodes on the path are
 * refused in the words of the five adjoint op nodes below, and images are what they were.  GAAST_OP_GLOG_ADJ2 (gaast_hip.h) is the
 * gradient in A of <g, GLOG_JVP(h, A)> with the roots of A held fixed, one node with three children like GAAST_OP_GEXP_ADJ2 (the third,
 * the forward operand, in input_slot): with both flags the family {GLOG_ADJ, GLOG_JVP, GLOG_ADJ2} is closed up to second order.
 * Errors: GAAST_ERR_INVALID_ARGUMENT for a wrt_slot out of range or const, or n_inputs + 1 > GAAST_MAX_INPUTS;
 * GAAST_ERR_UNIMPLEMENTED for one of the five adjoint op nodes on the path to wrt_slot, through either child (the message names the
 * op: the second derivative of these matrix functions needs Frechet-derivative kernels, which the library has for gexp alone and
 * uses under GAAST_FLAG_GEXP_GRAD2; under GAAST_FLAG_GSQRT_GLOG_JVP gsqrt's node is differentiated by composition and glog's with
 * respect to its cotangent, with GAAST_FLAG_GLOG_GRAD2 with respect to its operand too), and for GAAST_OP_GEXP_ADJ2 or
 * GAAST_OP_GLOG_ADJ2 on the path (third order);
 * GAAST_ERR_UNIMPLEMENTED for GAAST_FLAG_SPINOR_GEMM, and for exp / log on the path to wrt_slot unless desc->flags holds both
 * GAAST_FLAG_EXP_LOG and GAAST_FLAG_EXP_LOG_GRAD: then the operand's cotangent is a GAAST_OP_EXP_ADJ / GAAST_OP_LOG_ADJ node
 * (gaast_hip.h) over the cotangent of the exp / log node's buffer and the forward operand (exp of a bare scalar, grade set {0},
 * stays GAAST_ERR_UNIMPLEMENTED);
 * GAAST_ERR_INVALID_PROGRAM for a malformed desc.  The message is in gaast_expr_last_error(). */
int gaast_program_vjp(const gaast_program_desc *desc, int32_t wrt_slot, gaast_program_image_t *out);

/* number of input slots the program expects (caller slots + embedded constants) */
int gaast_spec_num_inputs(gaast_spec_t s);
int gaast_spec_num_user_inputs(gaast_spec_t s);

#ifdef __cplusplus
}
#endif
#endif /* GAAST_EXPR_H */
