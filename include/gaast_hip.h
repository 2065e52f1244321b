/*
 * gaast_hip.h -- C ABI of the MI355X (gfx950) back end for gaast's phase-4 evaluation.
 *
 * This is the drop-in boundary: it replaces the body of the reference's
 *     impl<T: GradedData + Debug> SpecializedAst<T> { pub fn eval<R: GradedDataMut>(&self) -> R }
 * (reference src/eval.rs:10-19) and the storage traits it evaluates over
 * (src/graded.rs:43-79).  Phases 1-3 (Expr operators, reify, specialize) stay on the host;
 * what crosses this boundary is exactly what the reference's public read API exposes after
 * phase 3 (src/ast/specialize.rs:17-24, src/ast/base_types.rs:8-55,124-146), flattened into
 * plain structs, plus per-grade component slabs.
 *
 * Conventions
 *  - every entry point returns a gaast_status (0 = OK); nothing aborts or throws across
 *    the ABI (the reference panics instead: see the GAAST_ERR_* comments);
 *  - one host thread drives the library (SpecializedAst is !Send + !Sync in the reference);
 *    calls are asynchronous on the library stream unless stated, gaast_hip_synchronize()
 *    or a download makes results visible;
 *  - the caller owns handles, the library owns the device memory behind them, no host
 *    pointer is retained after a call returns;
 *  - one process drives one GPU (one rank per GPU; multi-GPU batches shard by item: the
 *    "multi-GPU" section below is the only exchange between ranks);
 *  - the library's state (device, stream, communicator, scratch buffers) is per process and
 *    NOT synchronised: calls must come from one thread at a time.  Every entry point that
 *    touches the GPU makes the library's device current for the calling thread first, so the
 *    driving thread may change between calls (HIP's current device is per thread).
 *
 * Device storage of a batched multivector ("graded rows"): one row per batch item, a row
 * holds the dense per-grade component arrays of that item concatenated in ascending grade
 * order; within grade k the C(dim,k) components are in the reference's index order
 * (src/algebra.rs:221-246: colex rank of the blade's basis-vector set).  So the
 * reference's `grade_slice(k)` of item i is the contiguous run
 *     row(i)[ offset(k) .. offset(k) + C(dim,k) ).
 */
#ifndef GAAST_HIP_H
#define GAAST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GAAST_MAX_DIM 16   /* 2^16 components per full multivector; flat offsets fit 16 bits */
#define GAAST_MAX_INPUTS 64

typedef enum gaast_status {
    GAAST_OK = 0,
    GAAST_ERR_INVALID_PROGRAM = 1,  /* malformed flat program (reference: specialize.rs:104-117 asserts) */
    GAAST_ERR_MISSING_GRADE = 2,    /* reference panic: graded.rs:188,193 (grade absent from a buffer) */
    GAAST_ERR_UNIMPLEMENTED = 3,    /* reference panic: eval.rs:112-113 todo!() for exp / log; also returned by
                                     * gaast_hip_program_create for a program that is valid in the reference but
                                     * beyond this back end (e.g. a product whose operands exceed the LDS budget of
                                     * every kernel): such a program is refused whole, never half-evaluated */
    GAAST_ERR_HIP = 4,              /* a HIP runtime call failed; see gaast_hip_last_error() */
    GAAST_ERR_RCCL = 5,             /* an RCCL call failed / librccl could not be loaded / no communicator */
    GAAST_ERR_INVALID_ARGUMENT = 6,
    GAAST_ERR_NO_DEVICE = 7,        /* no gfx950 device / library not initialised */
    GAAST_ERR_OVERFLOW = 8          /* reference debug-build panic: eval.rs:90 `k - 1` with k == 0 */
} gaast_status;

typedef enum gaast_dtype {
    GAAST_F64 = 0, /* the reference's only value type (graded.rs:46) */
    GAAST_F32 = 1  /* extension used by the dense large-dimension configurations */
} gaast_dtype;

/* AstNode variants, reference src/ast/base_types.rs:8-30 (+ ScalarUnaryOp :84-88) */
typedef enum gaast_opcode {
    GAAST_OP_INPUT = 0,  /* GradedObj(T) */
    GAAST_OP_ADD = 1,    /* Addition */
    GAAST_OP_PRODUCT = 2,/* Product */
    GAAST_OP_NEG = 3,    /* Negation */
    GAAST_OP_EXP = 4,    /* Exponential (evaluation unimplemented upstream) */
    GAAST_OP_LOG = 5,    /* Logarithm   (evaluation unimplemented upstream) */
    GAAST_OP_PROJ = 6,   /* GradeProjection */
    GAAST_OP_REVERSE = 7,/* Reverse */
    GAAST_OP_GINVOL = 8, /* GradeInvolution */
    GAAST_OP_SINV = 9,   /* ScalarUnaryOp(Inversion) */
    GAAST_OP_SSQRT = 10, /* ScalarUnaryOp(SquareRoot) */
    /* Reverse mode of Exponential / Logarithm (no reference counterpart; gaast_program_vjp under GAAST_FLAG_EXP_LOG_GRAD emits
     * them, GAAST_FLAG_EXP_LOG evaluates them -- without that flag gaast_hip_program_create refuses a program that holds one:
     * GAAST_ERR_UNIMPLEMENTED).  They follow the pattern of GAAST_PROD_ADJ_*: child0 is the cotangent g of the forward node's
     * result (a node whose minimal grade mask lies within the forward node's: grade 0 and / or grade k), child1 the forward
     * operand, and the node's own minimal grade mask that of the operand (EXP_ADJ: {k}; LOG_ADJ: {0, k} or {k}).  Both nodes
     * ADD into the buffer that contains them, like every arm of eval.rs.  With sigma_i = e_i e_i, s = sum sigma_i B_i^2,
     * d = sum_i g_k[i] B_i over the grade-k components g holds, g_0 the scalar of g (0 when absent), and c0, f exactly as the
     * forward computes them (its s == 0 and NaN branches included):
     *   EXP_ADJ  dB_i = f g_k[i] + sigma_i B_i (f g_0 + h d),  h = (c0 - f) / s         (-> 1/3 at s = 0)
     *   LOG_ADJ  dB_i = f g_k[i] + sigma_i B_i h d,            h = (a / D - f) / s,  D = a^2 - s   (-> 2 / (3 a^3) at s = 0)
     *            da   = -d / D                                  (only when the operand holds grade 0)
     * h is summed from its series in s where the quotient cancels (DESIGN.md section 11 has the thresholds).  The adjoint does
     * NOT repeat the forward's domain check and never touches the domain-error counter; a VJP program that re-evaluates a
     * forward exp / log (because it needs its value, e.g. R in the sandwich R X ~R) counts there like any forward program.
     * Exp of a bare scalar (k = 0, raw ABI only) has no adjoint node: GAAST_ERR_UNIMPLEMENTED. */
    GAAST_OP_EXP_ADJ = 11,
    GAAST_OP_LOG_ADJ = 12,
    /* Complements (no reference counterpart; metric-free, so they work in a degenerate metric such as PGA's where a * I.rev() is
     * identically zero).  Blades are bitmasks S over n bits, ~S the complement of S, par(A,B) the parity of #{(i in A, j in B): i > j}:
     *   DUAL    right complement  dual(e_S)   = (-1)^par(S,~S) e_~S, so that e_S ^ dual(e_S) = I = e_{1..n};
     *   UNDUAL  left complement   undual(e_S) = (-1)^par(~S,S) e_~S, the exact inverse (and the transpose) of DUAL.
     * One child.  Component i of grade k goes to component C(n,k) - 1 - i of grade n - k (ascending bitmask within a grade), so the
     * node's minimal grade mask is the child's mirrored, k -> n - k.  Signed permutations: bit-exact in every mode and both dtypes;
     * like every arm of eval.rs the node ADDS +-x into the buffer that contains it, with one rounding.  An operand stored in another
     * dimension (a scalar literal: storage dimension 0) is taken as the leading components of the algebra's grades: a scalar
     * dualises to grade n of the algebra.  In a program of gaast_hip_program_create_in_basis the complement of the caller's basis is
     * det(Q) = +-1 times the one of the orthogonal basis: the library multiplies every sign by sign(det Q). */
    GAAST_OP_DUAL = 13,
    GAAST_OP_UNDUAL = 14,
    /* General multivector inverse (no reference counterpart): the Y with A Y = 1.  One child.  Let S be the even blades when the
     * child's minimal grade mask holds only even grades (the even subalgebra is closed), else all 2^n blades, N = |S|.  Y solves
     * L_A y = e_scalar with the left-multiplication matrix L_A[c][b] = coeff(a, b) A[a], a = c xor b (coeff: the blade-product sign
     * and metric factor of every product here; 0 where the child does not hold grade(a)); where A is invertible the left and right
     * inverses coincide.  The node's maximal grade set is {0, 2, 4, ... <= n} for an even child and {0 .. n} otherwise; it
     * produces the wanted grades of that set, while its child is wanted in ALL of the child's own grades.  Like every arm it ADDS
     * into the buffer that contains it.  A child whose mask is {0} is GAAST_OP_SINV (the expression layer lowers it so; the raw
     * ABI may carry GAAST_OP_INV on a scalar and gets the same launch as GAAST_OP_SINV).
     * Supported: N <= 64 (any mask for n <= 6, even masks for n = 7); beyond that gaast_hip_program_create returns
     * GAAST_ERR_UNIMPLEMENTED and creates nothing (phases 1-3 succeed on the host for any n).
     * Singular items: Gauss-Jordan elimination with partial pivoting; an item is singular when at any column the pivot p has
     * !(|p| > N eps max_i |A_i|) (eps of the program's dtype, max over the item's operand components; a NaN pivot is singular
     * too).  It is counted in gaast_hip_program_domain_errors (a program with an INV step owns the counter as one with exp / log
     * does) and every produced component of it is a quiet NaN.  An all-zero column gives an exact zero pivot: deterministic.
     * Non-finite inputs propagate as IEEE 754 dictates and may or may not be counted.
     * Accuracy: per non-singular item the normwise backward error ||L_A y - e||_inf / (||L_A||_inf ||y||_inf) <= 2 N eps to first
     * order (||L_A||_inf the largest absolute row sum): the scale of Gaussian elimination with partial pivoting.
     * GAAST_FLAG_EXACT_ORDER changes nothing here: there are no reference bits for an operation the reference lacks.
     * Reverse mode (gaast_program_vjp): with Y the inverse recomputed in every grade of S and g the cotangent of the node,
     * the child gets -ADJ_RIGHT_geometric(ADJ_LEFT_geometric(g, Y), Y), the adjoint of dA -> -(Y dA) Y. */
    GAAST_OP_INV = 15,
    /* General multivector exponential (no reference counterpart): gexp(A) = sum_k A^k / k! under the geometric product, for ANY
     * multivector -- GAAST_OP_EXP is a closed form that is only right for a single-grade k-vector whose square is a scalar.  One
     * child.  The blade set S, N = |S|, its ordering (S[j] = j, or (j << 1) | parity(j) for the even set) and the matrix
     * L_A[r][j] = coeff(r, j) A[r xor j] are those of GAAST_OP_INV; y = exp(L_A) e_scalar.  The node's maximal grade set is
     * GAAST_OP_INV's: {0, 2, 4, ...} for an even child, {0 .. n} otherwise; it produces the wanted grades of that set, its child is
     * wanted in all of the child's own grades, and like every arm it ADDS into the buffer that contains it.
     * Supported: N = 2 ... 64 (any mask for n <= 6, even masks for n = 7; not a bare scalar in a 0-dimensional algebra); anything
     * else is GAAST_ERR_UNIMPLEMENTED from gaast_hip_program_create, phases 1-3 succeeding on the host.  No flag gates the node and
     * GAAST_FLAG_EXACT_ORDER changes nothing: there are no reference bits.
     * Algorithm (scaling and squaring; every sum over j ascending), per item:
     *   1. theta = wmax * sum_a |A_a|, wmax the largest |metric factor| of the algebra (1 for +-1 / 0 metrics): theta >= ||L_A||_inf.
     *      The sum is a butterfly over the N components: v <- v + v[j xor m] for m = N/2, N/4, ... 1.
     *   2. s = the smallest integer >= 0 with theta 2^-s <= 1/2;  A_s = A 2^-s (exact).
     *   3. theta not finite, or s > 12 (theta > 2048): a domain error.  Every produced component of the item is a quiet NaN and the
     *      item is counted once in gaast_hip_program_domain_errors (a program with a GEXP step owns the counter).
     *   4. Taylor by Horner, degree m the smallest with (1/2)^(m+1) / (m+1)! <= eps / 2: m = 8 in f32, 14 in f64.
     *      q_m = e_0;  q_(k-1) = e_0 + (A_s q_k) / k  for k = m ... 1.
     *   5. Y_0 = q_0;  Y_(i+1) = Y_i Y_i for i < s;  the result is Y_s.
     * Accuracy: ||y - exp(A)||_inf <= 2 N eps max(1, theta) ||exp(A)||_inf per item that is no domain error. */
    GAAST_OP_GEXP = 16,
    /* Reverse mode of GAAST_OP_GEXP, emitted by gaast_program_vjp: child0 = the cotangent g of the GEXP node (any grades within
     * S), child1 = the forward operand A; the node's own minimal grade mask is the operand's.  It ADDS into its buffer; no flag.
     * The reverse sweep of the recurrences above, differentiating what is computed with s held fixed.  For P = X Z let
     *   ADJL(g, Z)[a] = sum_b coeff(a, b) Z[b] g[a xor b],   ADJR(g, X)[b] = sum_a coeff(a, b) X[a] g[a xor b],
     * coeff(a, b) the sign and metric factor of L[a xor b][b] (factor index S[a] & S[b]; degenerate metrics included).  Then
     *   g <- ADJL(g, Y_i) + ADJR(g, Y_i)  for i = s-1 ... 0;   dA_s = 0;
     *   for k = 1 ... m:  h = g / k;  dA_s += ADJL(h, q_k);  g <- ADJR(h, A_s);
     *   dA = 2^-s dA_s, restricted to the grades the operand holds.
     * The forward is recomputed.  No domain check and no count: a domain-error item of the forward has every component NaN (its
     * scaling factor is taken as NaN, so the arithmetic carries it). */
    GAAST_OP_GEXP_ADJ = 17,
    /* General multivector square root (no reference counterpart): gsqrt(A) is the PRINCIPAL square root, the X with X X = A whose
     * left-multiplication matrix L_X has every eigenvalue in the open right half plane.  It exists and is unique when L_A is
     * nonsingular and has no eigenvalue on the negative real axis; it is then a polynomial in A, so it lies in the blade set S of
     * GAAST_OP_INV and commutes with A.  The reference's sqrt (pow / exp / log behind GAAST_FLAG_EXP_LOG) is a closed form for
     * k-vectors whose square is a scalar and stays what it is.  One child.  S, N = |S|, its ordering and L_A are GAAST_OP_INV's; so
     * are the node's maximal grade set, the grades it produces and what it wants of its child, and like every arm it ADDS into the
     * buffer that contains it.  Supported: N = 2 ... 64 (any mask for n <= 6, even masks for n = 7); anything else is
     * GAAST_ERR_UNIMPLEMENTED from gaast_hip_program_create, phases 1-3 succeeding on the host (the expression layer lowers a scalar
     * operand to GAAST_OP_SSQRT).  No flag gates the node and GAAST_FLAG_EXACT_ORDER changes nothing: there are no reference bits.
     * Algorithm (the product form of the Denman-Beavers iteration, in multivector space: every iterate is a multivector over S;
     * every sum over j ascending), per item, with e_0 the scalar unit:
     *   M_0 = A, Y_0 = A;  for k = 0, 1, ...:
     *     d_k = sum_r |(M_k - e_0)_r|, a butterfly over the N components: v <- v + v[j xor m] for m = N/2, N/4, ... 1;
     *     stop (the result is Y_k) when d_k <= N eps, or when the step before had d_(k-1) <= sqrt(eps) (convergence is quadratic: one
     *     step past that point is at the rounding floor, where d_k itself may stagnate), or at k = K = 16;
     *     W = M_k^-1, the solve L_(M_k) W = e_0 of GAAST_OP_INV (Gauss-Jordan, implicit partial pivoting, the same pivot test
     *     !(|p| > N eps max_i |(M_k)_i|));
     *     Y_(k+1) = 1/2 (Y_k (e_0 + W));   M_(k+1) = 1/2 (e_0 + 1/2 (M_k + W)).
     * Domain errors: an item that meets a singular pivot in any inverse it runs, that has a non-finite d_k (a non-finite component),
     * or that has not stopped at k = K.  Every produced component of it is a quiet NaN and it is counted once in
     * gaast_hip_program_domain_errors (a program with a GSQRT step owns the counter).  -1, a vector (eigenvalues +-1), 0 and PGA's
     * ideal elements are such items by nature.
     * Accuracy: per item that is no domain error, the residual ||X X - A||_inf <= 9.2 N eps ||L_X||_inf ||X||_inf, which is four times
     * the worst of the numpy restatement of these recurrences over the test sweep (tests/gsqrt_numpy.py: FWD_SCALE = 2.3, measured
     * 2.12 in f32 and 2.24 in f64; operands gexp(B) with sum |B_i| <= 2.5 and operands with a dominant positive scalar), rounded up. */
    GAAST_OP_GSQRT = 18,
    /* Reverse mode of GAAST_OP_GSQRT, emitted by gaast_program_vjp: child0 = the cotangent g of the GSQRT node (any grades within
     * S), child1 = the forward operand A; the node's own minimal grade mask is the operand's.  It ADDS into its buffer; no flag.
     * From X X = A follows dX X + X dX = dA, so with GAAST_OP_GEXP_ADJ's operators the cotangent a of the operand is the solution
     * of the N x N system  ADJL(a, X) + ADJR(a, X) = g,  restricted to the grades the operand holds.  The operator is the transpose
     * of L_X + R_X: row c has, at column c xor t, coeff(c, t) X[t] once with ADJL's sign and once with ADJR's (exactly 0 where the
     * two blades anticommute); it is nonsingular whenever X is a principal root, no two eigenvalues of L_X summing to zero.  The
     * forward is recomputed, the system solved by GAAST_OP_INV's elimination.  A failed pivot test of this solve makes every
     * component of the item's cotangent NaN; it is not counted, and neither is a domain-error item of the recomputed forward, whose
     * cotangent is NaN likewise.  (A node whose own mask holds grades of S beyond the operand's produces those too -- the solution is
     * then restricted to the node's mask within S, not to the operand's grades: see GAAST_OP_GSQRT_JVP below, whose second-order rule
     * emits such nodes.  A node with the operand's mask, the only kind first-order reverse mode emits, is restricted as stated.) */
    GAAST_OP_GSQRT_ADJ = 19,
    /* General multivector logarithm (no reference counterpart): glog(A) is the PRINCIPAL logarithm, the Y with gexp(Y) = A whose
     * left-multiplication matrix L_Y has every eigenvalue in the strip |Im| < pi.  It exists and is unique when L_A is nonsingular
     * and has no eigenvalue on the negative real axis; it is then a primary function of A, lies in the blade set S of
     * GAAST_OP_INV and commutes with A.  The reference's log (behind GAAST_FLAG_EXP_LOG) is a closed form for k-vectors whose square
     * is a scalar and stays what it is.  One child.  S, N = |S|, its ordering and L_A are GAAST_OP_INV's; so are the node's maximal
     * grade set (GAAST_OP_GEXP's), the grades it produces and what it wants of its child (every grade it holds), and like every arm
     * it ADDS into the buffer that contains it.  There is no scalar lowering (no scalar-log opcode exists): a scalar operand is
     * evaluated over the even set, as GAAST_OP_GEXP does it.  Supported: N = 2 ... 64 (any mask for n <= 6, even masks for n = 7);
     * anything else is GAAST_ERR_UNIMPLEMENTED from gaast_hip_program_create, phases 1-3 succeeding on the host.  No flag gates the
     * node and GAAST_FLAG_EXACT_ORDER changes nothing: there are no reference bits.
     * Algorithm (inverse scaling and squaring, in multivector space: every iterate is a multivector over S; every sum over j
     * ascending), per item, with e_0 the scalar unit and wmax as GAAST_OP_GEXP defines it:
     *   X_0 = A, s = 0;
     *   while wmax * sum_r |(X_s - e_0)_r| > 1/4 (the butterfly sum of GAAST_OP_GSQRT) and s < S = 16:
     *     X_(s+1) = the principal root of X_s, exactly GAAST_OP_GSQRT's iteration (same stop rule, same K = 16 steps);  s += 1;
     *   E = X_s - e_0;   Y = sum_(j = 1 ... 7) alpha_j y_j,  y_j the solution of L_(e_0 + beta_j E) y_j = E,
     *     the [7/7] Pade approximant of log(1 + x) in partial fractions: alpha_j, beta_j are the weights and nodes of 7-point
     *     Gauss-Legendre quadrature on [0, 1] (gaast_amd/csrc/common/glog_pade.hpp).  Each term is one run of GAAST_OP_INV's
     *     elimination with right-hand side E and the pivot test !(|p| > N eps max_i |(e_0 + beta_j E)_i|): no inverse, no product;
     *   the result is 2^s Y (the factor is exact).
     * For ||L_E||_inf <= 1/4 the truncation error of the approximant is at most |r_7(-1/4) - log(3/4)| < 1e-16 (Kenney and Laub);
     * the same threshold 1/4 and degree 7 serve both value types.
     * Domain errors: an item with a non-finite component, with any domain error of a root it takes, still beyond 1/4 at s = S, or with
     * a failed pivot in a Pade solve.  Every produced component of it is a quiet NaN and it is counted once in
     * gaast_hip_program_domain_errors (a program with a GLOG step owns the counter).  -1, a vector (eigenvalues +-1), 0 and PGA's
     * ideal elements are such items by nature; so are unipotent items with sum |A - e_0| > 2^14 (1 + t e01 with a large t: each root
     * only halves t), a documented limitation and not a mathematical one.  The root's pivot test sets a second such limit: the
     * first root of 1 + t e01 meets the pivot 1 / t against N eps t, so the translator needs t^2 < 1 / (N eps) (in f32 over the 8
     * even blades of PGA3D: t < 1024).
     * Accuracy: per item that is no domain error, ||Y - log A||_inf <= 4 FWD_SCALE N eps max(1, sum_i |(log A)_i|), FWD_SCALE the
     * worst of the numpy restatement of these recurrences over the test sweep (tests/glog_numpy.py: FWD_SCALE = 8.0 in f32 and 7.5
     * in f64, measured 7.96 and 7.19, both on R^1; operands gexp(B) with sum |B_i| <= 2.5, operands with a dominant positive
     * scalar, and the former scaled by 37.5 and by 0.01: 0 ... 5 roots).  The reverse mode likewise: GRAD_SCALE = 2.3 / 2.0
     * (measured 2.20 / 1.95) in units of N eps max(1, sum_i |(log A)_i|) ||J^T||_inf ||g||_inf. */
    GAAST_OP_GLOG = 20,
    /* Reverse mode of GAAST_OP_GLOG, emitted by gaast_program_vjp: child0 = the cotangent g of the GLOG node (any grades within S),
     * child1 = the forward operand A; the node's own minimal grade mask is the operand's.  It ADDS into its buffer; no flag.
     * The forward is recomputed, keeping X_1 ... X_s.  Then, with GAAST_OP_GEXP_ADJ's operators:
     *   g' = 2^s g;
     *   a = sum_j alpha_j u_j,  where v_j solves R_(M_j)^T v_j = g' and u_j solves L_(M_j)^T u_j = v_j,  M_j = e_0 + beta_j E:
     *     the exact derivative of the approximant, d r(E) = sum_j alpha_j M_j^-1 dE M_j^-1 (the two solves commute).  Row c of
     *     R_M^T has coeff(c, t) M[t] with ADJL's sign at column c xor t, row c of L_M^T the same with ADJR's sign: the two halves of
     *     GAAST_OP_GSQRT_ADJ's row;
     *   for i = s ... 1:  a <- the solution of ADJL(a, X_i) + ADJR(a, X_i) = a, GAAST_OP_GSQRT_ADJ's system at X_i;
     *   a restricted to the grades the operand holds.
     * Every solve is GAAST_OP_INV's elimination, the pivot test against N eps max_i |M_i| of the multivector whose matrix it is.  A
     * failed pivot test, or a domain error of the recomputed forward, makes every component of the item's cotangent NaN; it is not
     * counted.  Accuracy: 4 GRAD_SCALE in the units GAAST_OP_GLOG states (tests/glog_numpy.py). */
    GAAST_OP_GLOG_ADJ = 21,
    /* The Frechet derivative L_A(h) of GAAST_OP_GEXP at A in direction h: the tangent of the recurrences above, s held fixed.
     * Emitted by gaast_program_vjp under GAAST_FLAG_GEXP_GRAD2 when it differentiates a GAAST_OP_GEXP_ADJ node with respect to its
     * cotangent; evaluating the node needs no flag.  child0 = the tangent h, which may hold only grades the operand holds (anything
     * else: GAAST_ERR_INVALID_PROGRAM); child1 = the forward operand A.  The node's own minimal grade mask lies within the maximal
     * grade set of GAAST_OP_GEXP over A (the grades it produces); it ADDS into its buffer.  Notation is GAAST_OP_GEXP's and
     * GAAST_OP_GEXP_ADJ's: S, N, coeff, ADJL, ADJR, wmax, the degree m, and s, which is computed from A alone.  With A_s, q_k, Y_i
     * the forward's and h_s = 2^-s h (exact):
     *   qd_m = 0;   qd_(k-1) = (h_s q_k + A_s qd_k) / k  for k = m ... 1   (two products, their sum, one division);
     *   Yd_0 = qd_0;   Yd_(i+1) = Yd_i Y_i + Y_i Yd_i  for i < s;   the result is Yd_s.
     * Every product is the forward's P[r] = sum_j L_X[r][j] Z[j], j ascending.  It is the transpose of GAAST_OP_GEXP_ADJ's sweep:
     * <g, GEXP_JVP(h, A)> = <GEXP_ADJ(g, A), h>.  No domain check and no count: a domain-error item of the forward takes its
     * scaling factor as NaN and every component of it comes back NaN by arithmetic.  Supported sizes are GAAST_OP_GEXP's. */
    GAAST_OP_GEXP_JVP = 22,
    /* The gradient with respect to A of <g, GEXP_JVP(h, A)>: the adjoint of the second Frechet derivative of GAAST_OP_GEXP, s held
     * fixed.  Emitted by gaast_program_vjp under GAAST_FLAG_GEXP_GRAD2; evaluating the node needs no flag.  child0 = g (any grades
     * within S), child1 = h (within the operand's grades, else GAAST_ERR_INVALID_PROGRAM), and a THIRD child, the forward operand A,
     * whose node index is carried in input_slot (a field no other opcode than GAAST_OP_INPUT uses: the node record and the wire
     * format keep their bytes).  The node's own minimal grade mask is the operand's; it ADDS into its buffer.
     * The pair (Y_i, Yd_i), (q_k, qd_k) of GAAST_OP_GEXP_JVP is recomputed.  Then, with Gd the cotangent of the tangent values and
     * G the cotangent of the values, both members of a pair computed from the old values:
     *   Gd = g, G = 0;
     *   for i = s-1 ... 0:  G  <- ((ADJL(G, Y_i) + ADJR(G, Y_i)) + ADJR(Gd, Yd_i)) + ADJL(Gd, Yd_i);
     *                       Gd <- ADJL(Gd, Y_i) + ADJR(Gd, Y_i);
     *   dA_s = 0;
     *   for k = 1 ... m:    w = G / k;  wd = Gd / k;
     *                       dA_s <- dA_s + (ADJL(w, q_k) + ADJL(wd, qd_k));
     *                       G  <- ADJR(w, A_s) + ADJR(wd, h_s);   Gd <- ADJR(wd, A_s);
     *   dA = 2^-s dA_s, restricted to the grades the operand holds.
     * No domain check and no count, as GAAST_OP_GEXP_JVP.  Supported sizes are GAAST_OP_GEXP's.
     * Accuracy of both, per item that is no domain error, against these recurrences in extended precision: 4 JVP_SCALE in units
     * of N eps max(1, theta) ||h||_inf ||exp A||_inf, and 4 ADJ2_SCALE in units of N eps max(1, theta) ||g||_inf ||h||_inf
     * ||exp A||_inf (tests/gexp2_numpy.py records the scales: the worst error of a numpy restatement in the program's dtype). */
    GAAST_OP_GEXP_ADJ2 = 23,
    /* The tangent of GAAST_OP_GSQRT at A in direction h, the transpose of GAAST_OP_GSQRT_ADJ's map.  Emitted by gaast_program_vjp under
     * GAAST_FLAG_GSQRT_GLOG_JVP; evaluating the node needs no flag.  child0 = the tangent h, which may hold any grades of the blade
     * set S of the operand (absent blades read as 0; grades outside S: GAAST_ERR_INVALID_PROGRAM); child1 = the forward operand A.
     * The node produces its own minimal grade mask within the grades of S; it ADDS into its buffer.  No third child.
     * With X the principal root of A, recomputed exactly as GAAST_OP_GSQRT_ADJ recomputes it (the same iteration, the same domain
     * rule), the result is the u with  (L_X + R_X) u = h,  that is  X u + u X = h:  row r of the system has at column j the value
     * w X[r xor j], w the metric factor of GAAST_OP_INV's L[r][j], once with the sign of L[r][j] = coeff(S[r] xor S[j], S[j]) and once
     * with the sign of the right-multiplication matrix R_X[r][j] = coeff(S[j], S[r] xor S[j]) X[r xor j].  One run of GAAST_OP_INV's
     * elimination, the pivot test !(|p| > N eps max_i |X_i|) of GAAST_OP_GSQRT_ADJ.  <g, GSQRT_JVP(h, A)> = <GSQRT_ADJ(g, A), h>.
     * No domain check and no count: a domain-error item of the recomputed forward, or a failed pivot, gives NaN in every produced
     * component.  Supported sizes are GAAST_OP_GSQRT's.  Accuracy, per item that is no domain error, against the same solve in
     * extended precision: 4 SQRT_JVP_SCALE in units of N eps kappa_inf(L_X + R_X) ||u||_inf (tests/root_log_jvp_numpy.py records
     * the scales: the worst error of a numpy restatement in the program's dtype).
     * A GAAST_OP_GSQRT_ADJ node whose own mask holds grades of S that the operand does not hold produces those too (its mask within
     * the grades of S, not within the operand's): the second-order rule of gaast_expr.h needs every component of the transposed
     * solve.  Every such node gaast_program_vjp emitted before that rule has the operand's mask, so nothing changes for those.
     * GAAST_OP_GEXP_ADJ and GAAST_OP_GLOG_ADJ keep the restriction to the operand's grades. */
    GAAST_OP_GSQRT_JVP = 24,
    /* The tangent of GAAST_OP_GLOG at A in direction h, the transpose of GAAST_OP_GLOG_ADJ's map; children, masks, flag and sizes as
     * GAAST_OP_GSQRT_JVP states them (sizes: GAAST_OP_GLOG's).  The roots X_1 ... X_s and s are taken from A alone, exactly as
     * GAAST_OP_GLOG_ADJ takes them, and held fixed.  Then
     *   t_0 = h;   (L_(X_i) + R_(X_i)) t_i = t_(i-1)  for i = 1 ... s, GAAST_OP_GSQRT_JVP's system at X_i;
     *   with E = X_s - e_0 and M_j = e_0 + beta_j E:  L_(M_j) p_j = t_s, then R_(M_j) q_j = p_j, for j = 1 ... 7
     *     (q_j = M_j^-1 t_s M_j^-1, the derivative of M_j^-1 E, since E commutes with M_j);
     *   the result is 2^s sum_j alpha_j q_j (j ascending; the factor is exact).
     * 14 non-transposed solves and s Sylvester solves: GAAST_OP_GLOG_ADJ read backwards.  Every solve is GAAST_OP_INV's elimination
     * with GAAST_OP_GLOG_ADJ's pivot tests.  <g, GLOG_JVP(h, A)> = <GLOG_ADJ(g, A), h>.  No domain check and no count: a domain-error
     * item of the recomputed forward, or a failed pivot, gives NaN in every produced component.  Accuracy: 4 LOG_JVP_SCALE in units
     * of N eps max(1, sum_i |(log A)_i|) ||J||_inf ||h||_inf (tests/root_log_jvp_numpy.py). */
    GAAST_OP_GLOG_JVP = 25,
    /* The gradient with respect to A of <g, GLOG_JVP(h, A)> = <GLOG_ADJ(g, A), h>: the adjoint of the second derivative of
     * GAAST_OP_GLOG, the roots X_1 ... X_s and s taken from A alone, exactly as GAAST_OP_GLOG_ADJ takes them, and held fixed.
     * Emitted by gaast_program_vjp under GAAST_FLAG_GSQRT_GLOG_JVP | GAAST_FLAG_GLOG_GRAD2; evaluating the node needs no flag.
     * child0 = g and child1 = h, each any grades of the blade set S of the operand (absent blades read as 0; grades outside S:
     * GAAST_ERR_INVALID_PROGRAM), and a THIRD child, the forward operand A, whose node index is carried in input_slot as
     * GAAST_OP_GEXP_ADJ2 carries it (the node record and the wire format keep their bytes).  The node's own minimal grade mask is the
     * operand's; it ADDS into its buffer.  With S_i = L_(X_i) + R_(X_i), E = X_s - e_0, M_j = e_0 + beta_j E and
     * ADJL(G, Z) = R_Z^T G, ADJR(G, X) = L_X^T G:
     *   up the chain:    t_0 = h;   S_i t_i = t_(i-1)  for i = 1 ... s  (GAAST_OP_GLOG_JVP's loop; every t_i is kept);
     *   scale:           g' = 2^s g  (exact);
     *   Pade, for j = 1 ... 7, j ascending, five solves per node:
     *                    R_(M_j)^T v1 = g';   L_(M_j)^T u = v1;   L_(M_j)^T v2 = g';   L_(M_j) p = t_s;   R_(M_j) q = p;
     *                    a <- a + alpha_j u                                      (GAAST_OP_GLOG_ADJ's first stage);
     *                    gamma <- gamma - alpha_j beta_j (ADJR(v1, q) + ADJL(v2, q))   (the adjoint of the second derivative of
     *                    the approximant: d(M^-1) = -beta M^-1 dE M^-1 on either side of q = M^-1 t_s M^-1);
     *   down the chain:  w = a, e = gamma;  for i = s ... 1:
     *                    w <- S_i^-T w;   e <- S_i^-T (e - (ADJR(w, t_i) + ADJL(w, t_i)))  with the new w
     *                    (d(S_i^-1) = -S_i^-1 (L_dX + R_dX) S_i^-1 and dX_i = S_i^-1 dX_(i-1));
     *   the result is e, restricted to the grades the operand holds.
     * 35 + 3 s eliminations; ADJR(., q) and ADJL(., q) are N multiply-adds each and no solve.  Every solve is GAAST_OP_INV's
     * elimination with GAAST_OP_GLOG_ADJ's pivot tests.  No domain check and no count, as GAAST_OP_GLOG_JVP: a domain-error item of
     * the recomputed forward, or a failed pivot, gives NaN in every produced component.  Supported sizes are GAAST_OP_GLOG's.
     * Accuracy, per item that is no domain error, against these recurrences in extended precision: 4 LOG_ADJ2_SCALE in units of
     * N eps max(1, sum_i |(log A)_i|) ||G||_inf ||h||_inf, G the N x N matrix with GLOG_ADJ2(g, h, A) = G h (tests/glog_adj2_numpy.py
     * records the scales: the worst error of a numpy restatement in the program's dtype). */
    GAAST_OP_GLOG_ADJ2 = 26
} gaast_opcode;

/* the five products of src/ast/expr.rs:180-197 (and the regressive product), for compact PRODUCT descriptors */
typedef enum gaast_product_kind {
    GAAST_PROD_EXPLICIT = -1, /* use the comp_muls list */
    GAAST_PROD_GEOMETRIC = 0,
    GAAST_PROD_OUTER = 1,
    GAAST_PROD_INNER = 2,
    GAAST_PROD_LCONTRACT = 3,
    GAAST_PROD_RCONTRACT = 4,
    /* the regressive product a v b = undual(dual(a) ^ dual(b)) (join of points / meet of planes; complements as GAAST_OP_DUAL).
     * On blades it is non-zero only when A | B is full; the result blade is A & B, of grade k_a + k_b - n, and the coefficient is
     * +-1 whatever the metric.  Its list (order T4, only the pairs with A | B full: 3^n entries for full multivectors) always runs on
     * the list kernels, never on a dense kernel.  With a Gram basis every coefficient is multiplied by sign(det Q), like the
     * complements. */
    GAAST_PROD_REGRESSIVE = 5,
    /* Compact ADJOINT products (reverse mode, gaast_program_vjp in gaast_expr.h): added to a forward kind 0..5, e.g.
     * GAAST_PROD_ADJ_LEFT + GAAST_PROD_GEOMETRIC.  child0 is the cotangent of the forward product's result, child1 the
     * other forward operand, and the node's own minimal grade mask that of the differentiated operand.  These three grade
     * sets regenerate the forward list (specialize.rs:132-183); the library evaluates its transpose: (l, r -> o, c) becomes
     * (o, r -> l, c) for ADJ_LEFT and (o, l -> r, c) for ADJ_RIGHT, forward order kept, ordered stably by result. */
    GAAST_PROD_ADJ_LEFT = 8,
    GAAST_PROD_ADJ_RIGHT = 16
} gaast_product_kind;

/* IndividualCompMul (base_types.rs:45-55) with Component{grade,index} (algebra.rs:87-91) */
typedef struct gaast_comp_mul {
    uint32_t left_grade, left_index;
    uint32_t right_grade, right_index;
    uint32_t result_grade, result_index;
    double coeff;
} gaast_comp_mul;

/* One GradedNode (base_types.rs:105-146): what eval.rs reads of it. */
typedef struct gaast_node_desc {
    int32_t opcode;              /* gaast_opcode */
    int32_t child0, child1;      /* indices of earlier nodes; -1 when unused */
    uint64_t minimal_grade_mask; /* GradedNode::grade_set(): bit k <=> grade k */
    int32_t vec_space_dim;       /* GradedNode::vec_space_dim() */
    int32_t input_slot;          /* OP_INPUT: which bound input */
    /* OP_PRODUCT, one of:
     *  - explicit: product_kind = GAAST_PROD_EXPLICIT and comp_muls[0..n_comp_muls) is
     *    Product.individual_comp_muls in the reference's order (specialize.rs:162-183);
     *  - compact: product_kind >= 0, comp_muls = NULL; the library regenerates the very same
     *    list from (kind, children's minimal sets, this node's minimal set, metric) by the
     *    rules of specialize.rs:132-183 / algebra.rs:73-83,199-246 -- or, for dense
     *    products, never materialises it. */
    int32_t product_kind;
    uint64_t n_comp_muls;
    const gaast_comp_mul *comp_muls;
} gaast_node_desc;

/* What eval.rs knows about a GradedObj(T): T::grade_set() and the slice lengths. */
typedef struct gaast_input_desc {
    uint64_t grade_mask;    /* Graded::grade_set() of the bound value */
    int32_t storage_dim;    /* slices have C(storage_dim,k) components; scalar literals use 0 (expr.rs:231-240) */
    int32_t is_const;       /* 1: value embedded below and shared by every batch item */
    const double *const_row;/* is_const: the row (grades ascending, concatenated) */
} gaast_input_desc;

#define GAAST_FLAG_DEBUG_OVERFLOW 0x1u /* reproduce the debug-build panic of eval.rs:90 (default: release) */
#define GAAST_FLAG_NO_FUSION 0x2u      /* one kernel per eval.rs arm, every operand materialised (A/B testing) */
/* Every sum in the reference's order with its three roundings per term (eval.rs:82): the result is the reference's, bit for bit.
 * WITHOUT the flag (the default) four things may differ, each within 4 eps sum |terms| per component (8: general metric) of the
 * reference's result OR closer to the exactly rounded sum than the reference's own sequential sum is:
 * dense products run on the re-ordered matrix-core kernels; long rows of a list product are summed in slices with fused
 * multiply-adds; a specialised small program whose arithmetic outweighs its bytes because an operand is SHARED by all items
 * (batch-1 input) contracts l * r + acc into one fused multiply-add; and the norm of a versor inverse / normalisation too big for
 * a fused program (n >= 9) is summed by the 64 lanes of a wave in parallel (the row is then read once).  Small programs over
 * batched operands and element-wise arms keep the reference's bits either way. */
#define GAAST_FLAG_EXACT_ORDER 0x4u
/* Reverse-mode programs (gaast_hip_program_create_vjp below) follow the same rule.  Default mode: an adjoint list is summed like
 * any forward list (slices with fused multiply-adds on long rows, contraction over shared operands), within the bound above of the
 * exactly rounded sum.  With EXACT_ORDER every adjoint list sums in the transposed table's order (result rows in ascending
 * component order, entries in forward order) with three roundings per term: the bits are the same on every run.  There are no
 * reference bits to match: the reference has no gradients. */
#define GAAST_FLAG_NO_MFMA 0x8u        /* dense products stay on the vector-FMA kernel (A/B testing) */
#define GAAST_FLAG_NO_JIT 0x10u        /* small programs run on the LDS interpreter kernel, not on hiprtc-specialised code */
/* OPT-IN, not the reference's algorithm: dense geometric products of a non-degenerate algebra (f32:
 * dimension 7..12, f32 and f64) go through the 2^m x 2^m complex matrix representation (at n = 12: 21x fewer
 * multiply-adds, all on the matrix cores).  Equal to eval.rs:61-86 in exact arithmetic; the error is bounded norm-wise,
 * |err_S| <= 64 eps(dtype) |A|_2 |B|_2, not per component.  Never selected without this flag. */
#define GAAST_FLAG_SPINOR_GEMM 0x20u
/* Debug hooks (explicit flags, no environment variables): */
#define GAAST_FLAG_DEBUG_JIT_FAILS 0x40u      /* treat every run-time (hiprtc) compilation as failed: exercises the fallbacks */
#define GAAST_FLAG_DEBUG_KEEP_JIT_SOURCE 0x80u /* keep the generated kernel source: gaast_hip_program_jit_source() */
/* OPT-IN extension with no reference behaviour (eval.rs:112-113 is todo!()): evaluate Exponential / Logarithm with the
 * semantics the grade rules imply (grade_set.rs:181-197), see DESIGN.md.  Without the flag such programs report
 * GAAST_ERR_UNIMPLEMENTED exactly where the reference panics. */
#define GAAST_FLAG_EXP_LOG 0x100u
/* OPT-IN, only meaningful together with GAAST_FLAG_EXP_LOG: reverse mode differentiates THROUGH Exponential / Logarithm
 * (gaast_program_vjp emits GAAST_OP_EXP_ADJ / GAAST_OP_LOG_ADJ nodes).  Without it -- GAAST_FLAG_EXP_LOG alone -- an exp / log
 * on the path to the differentiated input stays GAAST_ERR_UNIMPLEMENTED, and every status, plan, launch name and bit of a
 * program is what it was before the flag existed.  The flag changes nothing in a forward program. */
#define GAAST_FLAG_EXP_LOG_GRAD 0x2000u
/* OPT-IN: gaast_program_vjp differentiates THROUGH the adjoint family of the general exponential -- a GAAST_OP_GEXP_ADJ or
 * GAAST_OP_GEXP_JVP node on the path to the differentiated input gets GAAST_OP_GEXP_JVP / GAAST_OP_GEXP_ADJ / GAAST_OP_GEXP_ADJ2
 * nodes (table in gaast_expr.h): second-order reverse mode and forward mode through gexp.  Only gaast_program_vjp reads the flag;
 * the adjoint program inherits it like every flag.  Without it such a node stays GAAST_ERR_UNIMPLEMENTED, and every status, message,
 * plan, launch name and bit is what it was before the flag existed.  The flag changes nothing in a forward program, and in a
 * first-order VJP image only the flags word. */
#define GAAST_FLAG_GEXP_GRAD2 0x4000u
/* OPT-IN: gaast_program_vjp differentiates THROUGH the adjoint nodes of the general square root and logarithm.  A GAAST_OP_GSQRT_ADJ
 * or GAAST_OP_GSQRT_JVP node on the path to the differentiated input gets GAAST_OP_GSQRT_JVP / GAAST_OP_GSQRT_ADJ nodes and adjoint
 * products (table in gaast_expr.h): forward mode and reverse mode of any order through gsqrt.  A GAAST_OP_GLOG_ADJ or
 * GAAST_OP_GLOG_JVP node reached through child0 alone gets GAAST_OP_GLOG_JVP / GAAST_OP_GLOG_ADJ: forward mode through glog; one
 * whose operand depends on the differentiated input stays GAAST_ERR_UNIMPLEMENTED (unless GAAST_FLAG_GLOG_GRAD2 is set as well).  Only gaast_program_vjp reads the flag; the
 * adjoint program inherits it like every flag.  Without it such a node stays GAAST_ERR_UNIMPLEMENTED, and every status, message,
 * plan, launch name and bit is what it was before the flag existed.  The flag changes nothing in a forward program, and in a
 * first-order VJP image only the flags word. */
#define GAAST_FLAG_GSQRT_GLOG_JVP 0x8000u
/* OPT-IN, only meaningful together with GAAST_FLAG_GSQRT_GLOG_JVP: gaast_program_vjp differentiates a GAAST_OP_GLOG_ADJ or
 * GAAST_OP_GLOG_JVP node with respect to its OPERAND too, by one GAAST_OP_GLOG_ADJ2 node (table in gaast_expr.h): Hessian-vector
 * products and double backward through glog.  A GAAST_OP_GLOG_ADJ2 node on the path, third order, is GAAST_ERR_UNIMPLEMENTED.  Only
 * gaast_program_vjp reads the flag; the adjoint program inherits it like every flag.  Without it -- and with it alone -- every
 * status, message, image byte, plan and launch name is what it was before the flag existed. */
#define GAAST_FLAG_GLOG_GRAD2 0x10000u
#define GAAST_FLAG_DEBUG_LDS_12K 0x400u /* hiprtc-specialised kernels: 12 KiB instead of 10 KiB of LDS per wave for the row transposition (A/B testing) */
#define GAAST_FLAG_DEBUG_NO_CHAIN 0x800u /* a sparse product that only feeds a dense product stays a launch of its own (default: evaluated in the dense kernel's LDS staging; A/B testing) */
/* (bits 30 and 31 are reserved and ignored) */
#define GAAST_FLAG_DEBUG_FAIL_EVAL 0x1000u /* every evaluation of this program fails with GAAST_ERR_HIP before its first launch: exercises the failure path of gaast_hip_eval_gather on ONE rank */
#define GAAST_FLAG_NO_COALESCE 0x200u  /* hiprtc-specialised kernels: every lane reads / writes its own row (no LDS-transposed coalesced row I/O; A/B testing) */

typedef struct gaast_program_desc {
    int32_t vec_space_dim;      /* n */
    const double *metric_diag;  /* n squares of the base vectors (MetricAlgebra::base_vec_dot(i,i)) */
    int32_t dtype;              /* gaast_dtype of every buffer of this program */
    int32_t n_nodes;
    const gaast_node_desc *nodes; /* post-order: children before parents */
    int32_t root;               /* SpecializedAst::root_id() */
    int32_t n_inputs;
    const gaast_input_desc *inputs;
    uint32_t flags;
} gaast_program_desc;

typedef struct gaast_hip_program_s *gaast_hip_program_t;
typedef struct gaast_hip_mv_s *gaast_hip_mv_t;

/* ---- runtime ------------------------------------------------------------------------- */
/* Selects the GPU this process drives (device_ids[0]; n_dev must be 1: one rank per GPU -- a multi-GPU job is one
 * process per GPU joined by gaast_hip_comm_init below). */
int gaast_hip_init(const int *device_ids, int n_dev);
int gaast_hip_shutdown(void);
/* Launch on an existing HIP stream (e.g. torch's current stream); NULL = default stream. */
int gaast_hip_set_stream(void *hip_stream);
int gaast_hip_synchronize(void);
const char *gaast_hip_last_error(void);
const char *gaast_hip_version(void);

/* ---- SpecializedAst on the device ------------------------------------------------------ */
int gaast_hip_program_create(const gaast_program_desc *desc, gaast_hip_program_t *out);
int gaast_hip_program_destroy(gaast_hip_program_t prog);
/* grade mask / row length of the root result (root.minimal_grade_set) */
int gaast_hip_program_output_info(gaast_hip_program_t prog, uint64_t *grade_mask, int64_t *row_len);
/* number of kernel launches one eval issues, and a one-line description of launch `i` */
int gaast_hip_program_num_launches(gaast_hip_program_t prog);
const char *gaast_hip_program_launch_name(gaast_hip_program_t prog, int i);
/* Which of launch `i`'s kernels the most recent gaast_hip_eval of `prog` ran: the index into the launch's kernel table (the
 * alternatives its launch name lists as "0|1|2": picked at launch from the pointers and row strides of the bound rows; a
 * specialised program: 1 for its contracted build).  REDUCE_SCALE: 1 for k_reduce_scale_wave, 0 for k_reduce_scale.  0 for a
 * launch with a single kernel; negative before any evaluation and for a bad index.  Written on the host when the launch is
 * issued: forms chosen inside a kernel (gaast_jit, gaast_chain, k_linmap_small, k_sum_rows) are not visible here.  An
 * evaluation that is cut into item ranges (gaast_hip_eval_gather's chunks) issues every launch once per range, each with the
 * rows' base moved by first * stride -- which can change the alignment when the stride is not a multiple of 16 bytes: the value
 * is that of the LAST range.  Like every call on a program, to be made from the thread that drives it. */
int gaast_hip_program_launch_variant(gaast_hip_program_t prog, int i);
/* GAAST_FLAG_EXP_LOG extension: how many items, since the last call, had an exp / log operand outside the domain (a
 * k-vector whose square is not scalar: |<B B>_{not 0}|^2 > 2^-40 (sum B_i^2)^2); their results are the closed form applied
 * to <B B>_0 regardless.  A program with a GAAST_OP_INV step counts its singular items here too (their produced components are
 * NaN), one with a GAAST_OP_GEXP step its domain errors (theta not finite or > 2048; NaN likewise), one with a GAAST_OP_GSQRT step
 * the items without a principal root it can reach (GAAST_OP_GSQRT; NaN likewise), one with a GAAST_OP_GLOG step the items without a
 * principal logarithm it can reach (GAAST_OP_GLOG; NaN likewise).  Synchronises the library stream; resets the counter.  0 for
 * programs without exp / log / inv / gexp / gsqrt / glog. */
int gaast_hip_program_domain_errors(gaast_hip_program_t prog, int64_t *count);
/* GAAST_FLAG_DEBUG_KEEP_JIT_SOURCE: the HIP source generated for this program ("" if none). */
const char *gaast_hip_program_jit_source(gaast_hip_program_t prog);

/* ---- cache of compiled program kernels ------------------------------------------------------ */
/*
 * Small and medium programs run as kernels generated per program and compiled at gaast_hip_program_create (gaast_jit,
 * gaast_chain): set-up the reference's eval does not have (eval.rs:12-19 evaluates at once).  Compiled kernels are therefore
 * reused, on two levels, under one key: SHA-256 over the kernel revision gaast_hip_version() reports, the hiprtc version, the
 * target, every compile option, the entry point's name and the generated source (each field preceded by its length).
 *  - In the process, always: programs whose kernels have the same key share ONE loaded module, unloaded when the last of
 *    them is destroyed.  This changes the time of program creation only -- no launch name, no bit of any result.
 *  - In a directory, once the caller names one (the library reads no environment variable and writes no file otherwise): the
 *    code object exactly as the compiler returned it, so a later process loads the very code this one ran.
 *
 * File <dir>/<64 lower-case hex digits of the key>.gaastco, integers little-endian, no padding:
 *     offset   0   8 bytes   magic "GAASTCO\0"
 *     offset   8   uint32    format version (1)
 *     offset  12  32 bytes   kernel revision string, NUL-padded (its first 32 bytes if longer)
 *     offset  44  32 bytes   the key
 *     offset  76   uint64    payload length L; the file is exactly 116 + L bytes long
 *     offset  84  32 bytes   SHA-256 of the payload
 *     offset 116   L bytes   payload: the code object as hiprtcGetCode returned it
 * A file is written under a temporary name in the same directory (<final name>.tmp.<pid>.<serial>) and renamed onto its
 * final name, so concurrent writers (the ranks of a launch) leave one complete file.  A file that fails any check on load
 * (magic, version, revision, key, length against its size, payload hash) is never used: the kernel is compiled and the file
 * replaced.  Failures to write are ignored; program creation never fails because of the cache.  Only successful compilations
 * are stored.  Nothing is ever evicted.
 */
/* Turns the directory level on (eval.rs:12-19 has no set-up; this keeps ours to the first process).  NULL or "": off.
 * Otherwise the last component of `path` is created when missing; GAAST_ERR_INVALID_ARGUMENT, and the level off, when it
 * cannot be created or is not a directory.  Needs neither gaast_hip_init nor a GPU. */
int gaast_hip_jit_cache_set_dir(const char *path);
typedef enum gaast_jit_cache_counter {
    GAAST_JIT_CACHE_COMPILED = 0,      /* kernels compiled by hiprtc (successfully) */
    GAAST_JIT_CACHE_MEMORY_HITS = 1,   /* kernels taken from a module already loaded in this process */
    GAAST_JIT_CACHE_DISK_HITS = 2,     /* kernels loaded from a checked file of the directory */
    GAAST_JIT_CACHE_DISK_STORES = 3,   /* files written (renamed into place) */
    GAAST_JIT_CACHE_DISK_REJECTED = 4, /* files found and not used: a failed check, or a code object HIP refused */
    GAAST_JIT_CACHE_LIVE_MODULES = 5,  /* modules loaded now (the one counter that also falls) */
    GAAST_JIT_CACHE_N_COUNTERS = 6
} gaast_jit_cache_counter;
/* How much of program creation's set-up (absent from eval.rs:12-19) was compilation: fills out[0 .. min(n, count)) with the
 * process's counters in the order of gaast_jit_cache_counter and returns how many counters exist (never an error; out may be
 * NULL with n = 0).  Needs neither gaast_hip_init nor a GPU. */
int gaast_hip_jit_cache_stats(int64_t *out, int n);

/* ---- GradedDataMut on the device (graded.rs:51-79) ------------------------------------- */
/* init_null_mv(dim, gs) for `batch` items: zero-filled rows (graded.rs:195-201). */
int gaast_hip_mv_alloc(int dim, uint64_t grade_mask, int64_t batch, int dtype, gaast_hip_mv_t *out);
/* Same layout over caller-owned device memory (e.g. a torch tensor); row_stride in elements.  device_ptr must be a multiple of
 * the element size (GAAST_ERR_INVALID_ARGUMENT otherwise, nothing is created); any further alignment only decides which row
 * I/O form of a kernel runs. */
int gaast_hip_mv_wrap(void *device_ptr, int dim, uint64_t grade_mask, int64_t batch, int dtype,
                      int64_t row_stride, gaast_hip_mv_t *out);
int gaast_hip_mv_free(gaast_hip_mv_t mv);
int gaast_hip_mv_info(gaast_hip_mv_t mv, int *dim, uint64_t *grade_mask, int64_t *batch, int *dtype,
                      int64_t *row_len, int64_t *row_stride, void **device_ptr);
/* grade_slice_mut(k) of every item <- host[batch][C(dim,k)] (values in the mv's dtype). Synchronous. */
int gaast_hip_mv_upload(gaast_hip_mv_t mv, int grade, const void *host, int64_t count);
/* host[batch][C(dim,k)] <- grade_slice(k) of every item. Synchronous. */
int gaast_hip_mv_download(gaast_hip_mv_t mv, int grade, void *host, int64_t count);
/* whole rows at once: host[batch][row_len] */
int gaast_hip_mv_upload_rows(gaast_hip_mv_t mv, const void *host, int64_t count);
int gaast_hip_mv_download_rows(gaast_hip_mv_t mv, void *host, int64_t count);
int gaast_hip_mv_zero(gaast_hip_mv_t mv);

/* ---- SpecializedAst::eval (eval.rs:12-19), batched --------------------------------------- */
/*
 * Evaluates `prog` once per batch item.  inputs[slot] binds the GradedObj of that slot
 * (const slots may be NULL); an input whose batch is 1 is shared by all items.  `out` must
 * have the root's grade mask (gaast_hip_program_output_info) and `batch` items; it is
 * overwritten (the reference returns a fresh R).
 */
int gaast_hip_eval(gaast_hip_program_t prog, const gaast_hip_mv_t *inputs, int n_inputs,
                   int64_t batch, gaast_hip_mv_t out);

/* ---- non-diagonal metrics and linear maps of the vector space ------------------------------ */
/*
 * The reference's MetricAlgebra is a full Gram matrix (algebra.rs:57-66); its product rule assumes it diagonal (algebra.rs:68-83).
 * A Gram metric G = Q diag(L) Q^T (gaast_metric_diagonalize, include/gaast_expr.h) is evaluated in the orthogonal basis
 * f_j = sum_i Q_ij e_i, whose metric diag(L) every kernel handles: specialise the program for diag(L), then create it with
 * gaast_hip_program_create_in_basis.  Rows cross the boundary in the caller's basis e.
 *
 * The change of basis is the outermorphism of a linear map M of the vector space: on grade k of a row, the k-th compound C_k(M)
 * (gaast_compound_matrix), shared by every item -- also public, as a linear map applied to a batch of multivectors.
 * Linear maps and in-basis programs accept n <= 14 (the compounds at n = 14 total C(28,14) ~ 40 M entries); beyond that they
 * return GAAST_ERR_UNIMPLEMENTED and nothing is created.
 */
typedef struct gaast_hip_linmap_s *gaast_hip_linmap_t;
/* matrix: n x n, row-major, finite.  The compounds of every grade are built once on the host (f64, rounded to dtype) and
 * uploaded.  Synchronous. */
int gaast_hip_linmap_create(int n, const double *matrix, int dtype, gaast_hip_linmap_t *out);
/* out(item)_k = C_k(M) in(item)_k for every grade k of the rows.  in and out: dimension n, the map's dtype, the same grade mask
 * and batch, no overlap (rows may be strided: gaast_hip_mv_wrap).  Asynchronous on the library stream. */
int gaast_hip_linmap_apply(gaast_hip_linmap_t map, gaast_hip_mv_t in, gaast_hip_mv_t out);
/* The adjoint of gaast_hip_linmap_apply with respect to the rows: out(item)_k = C_k(M)^T in(item)_k.  C_k(M)^T = C_k(M^T), so this is
 * gaast_hip_linmap_apply of the map of M^T, bit for bit: the same kernels on a second set of compounds, built (synchronously, like
 * gaast_hip_linmap_create) at the first call and owned by the map.  Arguments, limits and asynchrony as gaast_hip_linmap_apply. */
int gaast_hip_linmap_apply_transposed(gaast_hip_linmap_t map, gaast_hip_mv_t in, gaast_hip_mv_t out);
/* The adjoint with respect to the matrix.  in = x and cotangent = g: dimension n, the map's dtype, the same grade mask and batch B >= 1.
 * For L = sum_items sum_k <g_k, C_k(M) x_k> it writes dL/dM, n x n elements of the map's dtype, row-major, to dmatrix_dev (device
 * memory that overlaps neither rows):
 *   W_k[I][J] = sum_items g_k[item][I] x_k[item][J]                                             (k_linmap_outer_sum)
 *   dL/dM[i][j] = sum_{k >= 1} sum_{I has i, J has j} (-1)^(p_I(i) + p_J(j)) C_{k-1}(M)[I \ i][J \ j] W_k[I][J]     (k_linmap_minor_contract)
 * as gaast_compound_matrix_vjp (gaast_expr.h) states it; grade 0 contributes nothing.  n <= 8 only (W has C(2n,n) entries: 12,870 at
 * n = 8, 2.7 M at n = 12): beyond that GAAST_ERR_UNIMPLEMENTED and nothing is written.
 * Deterministic, no atomics: W is summed over the items in item order within chunks of GAAST_SUM_ROWS_CHUNK items (a chain of fused
 * multiply-adds on the matrix cores, four items per instruction, added in item order), then the chunk partials in chunk order
 * (k_sum_rows); each entry of dL/dM then sums its terms -- ordered by k, I, J -- in 256 interleaved chains (term t in chain t mod 256)
 * joined by a fixed binary tree.  The bits depend on B, the grade mask and the data only.  Everything accumulates in the dtype:
 *   |result - exact| <= (d + 4) eps sum |terms| per entry, to first order,
 *   d = min(B, GAAST_SUM_ROWS_CHUNK) + ceil(B / GAAST_SUM_ROWS_CHUNK) + 22
 * (22 = ceil(C(14,7) / 256) + 8: the longest chain and the tree of the contraction at n = 8), |terms| = |C_{k-1} entry| |g| |x|, with
 * the compounds as the map holds them (rounded to the dtype from double).
 * Scratch as gaast_hip_mv_sum_rows: W and its chunk partials live in the library's per-stream reduction buffer, grown on first use
 * with a larger size after synchronising that stream -- so the first such call on a stream must not be inside a stream capture; the
 * term table of a grade mask is built and uploaded (synchronously) the first time the map sees that mask.  Otherwise asynchronous on
 * the library stream, no host synchronisation. */
int gaast_hip_linmap_matrix_vjp(gaast_hip_linmap_t map, gaast_hip_mv_t in, gaast_hip_mv_t cotangent, void *dmatrix_dev);
int gaast_hip_linmap_destroy(gaast_hip_linmap_t map);
/* desc: a program specialised for the orthogonal basis f (its metric_diag is L; explicit comp-mul lists computed in f are fine).
 * basis: Q as gaast_metric_diagonalize returns it, refused (GAAST_ERR_INVALID_ARGUMENT) unless |Q^T Q - I| <= 1e-12 elementwise.
 * Inputs are bound and the result written in the caller's basis e: every batched input slot with grades above 0 goes through
 * C_k(Q^T) into library scratch first (one scratch row per item per such slot, grown with the batch; an input shared by all items
 * is moved once per evaluation), constant inputs are moved on the host here, and the result comes back through C_k(Q) -- launches
 * "linmap[...]" in gaast_hip_program_launch_name.  Q == I exactly: the very program (plan, launches, bits) of
 * gaast_hip_program_create.  GAAST_FLAG_EXACT_ORDER applies to the program inside the basis change: there are no reference bits
 * in a non-diagonal metric. */
int gaast_hip_program_create_in_basis(const gaast_program_desc *desc, const double *basis, gaast_hip_program_t *out);

/* ---- multi-GPU: one rank per GPU, batch sharded by item ------------------------------------ */
/*
 * The reference evaluates one input set per eval() and keeps no cross-item state (eval.rs:16), so a batch
 * shards into contiguous item ranges with no data-path collective; the ONLY exchange is the gather of the
 * result rows to one rank.  The library does that itself over RCCL (xGMI), so that a non-Python host (the
 * Rust shim) needs nothing else: rank 0 calls gaast_hip_comm_unique_id and ships the 128 bytes to the other
 * ranks by any channel (file, socket, MPI, torch.distributed); every rank then calls gaast_hip_comm_init
 * (collective).  librccl is loaded on first use (dlopen), not at link time.
 */
#define GAAST_COMM_ID_BYTES 128
/* Which shared object provides the nccl* entry points the gather uses (ncclGetUniqueId, ncclCommInitRank,
 * ncclCommDestroy, ncclSend, ncclRecv, ncclAllReduce, ncclGroupStart, ncclGroupEnd, ncclGetErrorString): NULL = the
 * system's librccl (default: soname lookup, then /opt/rocm/lib).  For hosts that ship their own RCCL build and for the
 * test transport that lets several ranks share one GPU (tests/cpp/rccl_stub.c).  Call before the first
 * gaast_hip_comm_* use; GAAST_ERR_RCCL once another library has been loaded. */
int gaast_hip_comm_set_library(const char *path);
int gaast_hip_comm_unique_id(void *id_out);
int gaast_hip_comm_init(const void *id, int rank, int world);
int gaast_hip_comm_destroy(void);
/* rank / world of the communicator (GAAST_ERR_RCCL if there is none) */
int gaast_hip_comm_info(int *rank, int *world);
/* all-reduce(sum) of one 1 per rank over the communicator: how many ranks RCCL actually joined (synchronous) */
int gaast_hip_comm_count_ranks(int *n_ranks);
/*
 * Gather result rows to `root`: rank r contributes the first counts[r] rows of `local` (contiguous rows:
 * row_stride == row_len); on root, `gathered` receives them in rank order (item order of the global batch),
 * rank r's rows starting at row counts[0] + ... + counts[r-1].  `gathered` is ignored on the other ranks (may
 * be NULL).  The root receives from all peers concurrently (one direct peer-to-peer transfer per xGMI link,
 * not a ring).  Asynchronous on the library streams like gaast_hip_eval.
 */
int gaast_hip_gather_rows(gaast_hip_mv_t local, gaast_hip_mv_t gathered, const int64_t *counts, int root);
/*
 * gaast_hip_eval + gather, overlapped: the local batch (counts[rank] items) is evaluated in `n_chunks`
 * contiguous chunks and chunk k travels to `root` on a second stream while chunk k+1 is being computed.
 * Equivalent to gaast_hip_eval(prog, inputs, n_inputs, counts[rank], out) followed by
 * gaast_hip_gather_rows(out, gathered, counts, root).  `out` may be the rows of `gathered` that belong to the
 * root itself (same device memory): the local copy is then skipped.
 * FAILURE IS COLLECTIVE: a rank whose evaluation fails after the argument checks (a launch error) still posts
 * its transfers, so that no peer is left waiting in a receive, and before returning every rank all-reduces an
 * error flag over the communicator: if ANY rank failed, EVERY rank returns non-zero (the failing rank its own
 * status, the others GAAST_ERR_RCCL "another rank failed") and the contents of `gathered` are unspecified.  The
 * flag exchange makes this entry point synchronous with the communicator's stream: when it returns GAAST_OK
 * the gathered rows have arrived.  (Argument errors are detected before any transfer and are the caller's to
 * keep consistent across ranks: the same counts / root / n_chunks everywhere.)
 */
int gaast_hip_eval_gather(gaast_hip_program_t prog, const gaast_hip_mv_t *inputs, int n_inputs,
                          gaast_hip_mv_t out, gaast_hip_mv_t gathered, const int64_t *counts, int root,
                          int n_chunks);

/* ---- reverse mode ------------------------------------------------------------------------------ */
/* gaast_program_vjp (gaast_expr.h) followed by gaast_hip_program_create.  Bind slots 0 .. desc->n_inputs - 1 as for the forward
 * program and the cotangent (root grade mask, dimension n, one row per item) at slot desc->n_inputs; gaast_hip_eval writes the
 * gradient rows of input `wrt_slot` (its grade mask and storage dimension).  Batch-1 inputs are shared as usual; the gradient of a
 * shared input is then one row per item, to be summed with gaast_hip_mv_sum_rows.  Programs created with
 * GAAST_FLAG_SPINOR_GEMM have no VJP: GAAST_ERR_UNIMPLEMENTED; so has an exp / log on the path to `wrt_slot` unless desc->flags holds
 * GAAST_FLAG_EXP_LOG | GAAST_FLAG_EXP_LOG_GRAD.  A program of gaast_hip_program_create_in_basis has the VJP below.
 * desc may itself be a VJP program (read from the image of gaast_program_vjp): gaast_program_vjp is closed under itself, so this
 * creates second- and higher-order programs, the cotangent of desc being one of its slots and wrt_slot any non-const one.  Adjoint
 * products of dense geometric products run on the forward's dense kernels at every order.  One of the adjoint op nodes
 * (GAAST_OP_EXP_ADJ, LOG_ADJ, GEXP_ADJ, GSQRT_ADJ, GLOG_ADJ) on the path to wrt_slot: GAAST_ERR_UNIMPLEMENTED -- except GEXP_ADJ (and
 * GEXP_JVP) when desc->flags holds GAAST_FLAG_GEXP_GRAD2: second order and forward mode through gexp (gaast_expr.h has the table);
 * a GAAST_OP_GEXP_ADJ2 node on the path, third order, is GAAST_ERR_UNIMPLEMENTED.  GSQRT_ADJ / GSQRT_JVP (any order) and GLOG_ADJ /
 * GLOG_JVP (through child0: forward mode) differentiate when desc->flags holds GAAST_FLAG_GSQRT_GLOG_JVP; with GAAST_FLAG_GLOG_GRAD2
 * beside it GLOG_ADJ / GLOG_JVP differentiate through their operand too (one GAAST_OP_GLOG_ADJ2 node: second order through glog),
 * and a GAAST_OP_GLOG_ADJ2 node on the path, third order, is GAAST_ERR_UNIMPLEMENTED. */
int gaast_hip_program_create_vjp(const gaast_program_desc *desc, int32_t wrt_slot, gaast_hip_program_t *out);
/* gaast_program_vjp followed by gaast_hip_program_create_in_basis: the VJP of a program in a non-diagonal metric.  With the orthogonal
 * Q of the basis change, y_e = C(Q) F(C(Q^T) x_e) and every C_k(Q) is orthogonal, so the VJP of the in-basis program is the in-basis
 * version of the VJP program with the same Q: the cotangent (slot desc->n_inputs, an ordinary batched input of dimension n) goes
 * through C_k(Q^T) like every other input, the gradient comes back through C_k(Q).  desc is the FORWARD program specialised for
 * diag(L), its constant rows in the caller's basis exactly as gaast_hip_program_create_in_basis takes them.  Q == I exactly: the very
 * program (plan, launches, bits) of gaast_hip_program_create_vjp.  desc may also be a VJP program of such a forward program, with the
 * same Q: every level of a higher-order program is the in-basis version of the plain one, all rows in the caller's basis.
 * A wrt_slot whose rows hold only grade 0 gets no result move.  The
 * exp / log adjoint nodes work unchanged inside f (sigma_i is the metric of f there).  Errors: those of gaast_program_vjp
 * (GAAST_FLAG_SPINOR_GEMM stays GAAST_ERR_UNIMPLEMENTED) and of gaast_hip_program_create_in_basis; *out is untouched on failure. */
int gaast_hip_program_create_vjp_in_basis(const gaast_program_desc *desc, const double *basis, int32_t wrt_slot,
                                          gaast_hip_program_t *out);
/* out(0) = sum over the B rows of `in` (out: batch 1, same dimension, grade mask and dtype; B >= 1).  Deterministic: rows are
 * summed in index order within chunks of GAAST_SUM_ROWS_CHUNK rows, then the chunk partials in chunk order, so the bits depend
 * on B and the data only.  Sums accumulate in the dtype (f32 in f32): |result - exact| <= (GAAST_SUM_ROWS_CHUNK - 1 + ceil(B /
 * GAAST_SUM_ROWS_CHUNK)) eps sum_i |x_i| per component, to first order.  No atomics; the partials live in library scratch, one
 * buffer per stream (B > GAAST_SUM_ROWS_CHUNK), grown on first use with a larger row count after synchronising that stream -- so
 * the first such call on a stream must not be inside a stream capture.  in and out must not overlap.  Asynchronous on the library
 * stream. */
#define GAAST_SUM_ROWS_CHUNK 1024
int gaast_hip_mv_sum_rows(gaast_hip_mv_t in, gaast_hip_mv_t out);

#ifdef __cplusplus
}
#endif
#endif /* GAAST_HIP_H */
