// Lowering of a flat SpecializedAst program into a launch plan that reproduces the control
// flow of the reference's interpreter (src/eval.rs:12-115) arm by arm.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../common/algebra.hpp"
#include "../common/comp_mul_table.hpp"
#include "dense_images.hip.hpp"
#include "explog_adj_series.hip.hpp"
#include "gaast_hip.h"

namespace gaast {

enum class BufKind : int { NODE = 0, INPUT = 1, OUT = 2 };

struct BufRef {
    BufKind kind = BufKind::NODE;
    int idx = -1;  // NODE: cache-buffer id; INPUT: slot; < 0: no buffer
};
inline bool operator==(BufRef x, BufRef y) { return x.kind == y.kind && x.idx == y.idx; }
inline bool operator!=(BufRef x, BufRef y) { return !(x == y); }

struct Layout {  // how a graded row is laid out
    int dim = 0;
    uint64_t mask = 0;
    int64_t row_len = 0;
    int64_t offset(int k) const { return grade_offset(dim, mask, k); }
    int64_t grade_len(int k) const { return int64_t(n_choose_k(uint64_t(dim), uint64_t(k))); }
};

inline Layout make_layout(int dim, uint64_t mask) {
    Layout l;
    l.dim = dim;
    l.mask = mask;
    l.row_len = row_len_of(dim, mask);
    return l;
}

// (DenseFamily, which kernel family runs a PRODUCT_DENSE step: dense_images.hip.hpp, with the families' operand images)

// One launch of the plan.  What every step has comes first; then one group of fields per step kind (and per rewrite a pass applies to
// a step in place), each table and setting named after the one thing it holds.  The groups of the other kinds stay empty.  The
// tables are host images, uploaded once at program_create.
struct Step {
    enum Kind { ZERO, AXPY, FLIP, SUNARY, PRODUCT_CSR, PRODUCT_DENSE, FUSED, EXPLOG, REDUCE_SCALE, ELEMENTWISE, LINMAP, EXPLOG_ADJ, DUAL, INVERSE, GEXP, GEXP_ADJ, GSQRT, GSQRT_ADJ, GLOG, GLOG_ADJ, GEXP_JVP, GEXP_ADJ2, GSQRT_JVP, GLOG_JVP, GLOG_ADJ2 } kind = ZERO;
    BufRef res, a, b;        // result; operand rows (PRODUCT_*: left, right; AXPY / EXPLOG / LINMAP / DUAL / INVERSE / GEXP / GSQRT / GLOG: a; EXPLOG_ADJ / GEXP_ADJ / GSQRT_ADJ / GLOG_ADJ: a = the forward operand, b = the cotangent; REDUCE_SCALE: the reduction's; ELEMENTWISE: b = the scalar)
    BufRef c;                // a third operand row (GEXP_JVP / GSQRT_JVP / GLOG_JVP: a = the forward operand, c = the tangent h; GEXP_ADJ2 / GLOG_ADJ2: a, b = g, c = h)
    std::string name;
    int canon_a = 0, canon_b = 0;   // the operand is a bound input read in place: the kernel applies the reference's 0.0 + x
    int beta = 1;                   // 0: the zero fill of a fresh result is folded in
    uint64_t n_entries = 0;         // comp-mul count this step stands for

    std::vector<uint32_t> axpy_map;       // AXPY: result offset | operand offset << 16
    std::vector<uint32_t> flip_offsets;   // FLIP: result offsets
    int sunary_op = 0, sunary_off = 0;    // SUNARY: 0 1 / s, 1 sqrt(s); offset of grade 0

    // PRODUCT_CSR: the comp-mul list by result component, entries in the reference's order
    struct List {
        std::vector<uint32_t> row_start;   // rows + 1
        std::vector<uint32_t> row_out;     // result offset of each row
        std::vector<uint32_t> entries;     // left offset | right offset << 16
        std::vector<double> coeff;         // (converted to the program dtype on upload)
        int ell_width = 0;                 // > 0: rows of one length with +-1 coefficients: entries is [term][row], sign in bit 31, no row_start / coeff
        int ell_bytes = 0;                 // ... and the offsets of its entries are byte offsets
    } list;

    // PRODUCT_DENSE
    struct Dense {
        DenseFamily family = DenseFamily::VECTOR_FMA;
        int n = 0;   // dimension of the algebra the kernel runs in (the program's n, or n - 1: parity-pure operands)
        std::vector<uint32_t> left_map, right_map;   // row offset | image position << 16 | negate << 31 (SPINOR: 16-bit entries, two per word)
        std::vector<int32_t> out_map;                // by blade of the permuted basis: offset | sign << 30, or -1
        std::vector<uint32_t> spinor_out_map;        // SPINOR: 16-bit entries, two per word
        // a general diagonal metric (entries other than +-1 / 0): the kernels run in the rescaled basis f_i = e_i / sqrt|g_i|:
        // w_S per loaded left / right component, 1 / w_T per blade of the permuted basis (the index of out_map)
        std::vector<double> left_scale, right_scale, out_scale;
        int scaled = 0;
        int left_full = 0, right_full = 0, out_full = 0;
        int left_contig = 0, right_contig = 0;
        int left_signs = 0, out_signs = 0;   // some left_map word negates / some out_map word carries a reordering sign
        int right_signs = 0;                 // some right_map word negates (the image signs of the B side, folded sign arms)
        int out_all = 0;                     // every blade of the permuted basis is produced: no out_map word is -1
        uint32_t neg_hi = 0, zero_hi = 0;
        uint32_t neg_lo = 0;   // lo basis vectors (of the permuted basis) that square to -1
        int neg_lo_all = 0;    // vector-FMA kernel: the NEGLO instantiation (all four lo vectors square to -1)
        int degenerate = 0;
        int mfma16_quads = 0;  // MFMA16X4 in f32: the B image in the 16-byte-quad layout
        int spinor_lam_bit = -1, spinor_has_alpha = 0;  // index basis of the matrix-representation kernels: spinor_basis.hpp
        int spinor_m = 0;      // SPINOR: log2 of the matrix size
        // (plan_passes.cpp: chain_sparse_into_dense): the LEFT operand is the result of a short comp-mul list over two other rows
        // (eval.rs:61-86 with a cached operand that nothing else reads: R X in R X ~R) -- `pre`.  The list is evaluated in LDS while
        // the dense kernel stages its operands -- reference order, same roundings -- and the intermediate never goes through HBM.
        int chained = 0;
    } dense;

    // The list evaluated in LDS ahead of a dense product (dense.chained: its rows are components of the left image) or ahead of a
    // second list (chain.side: its rows are elements of the mid row)
    struct Pre {
        BufRef a, b;                      // the list's operand rows
        int canon_a = 0, canon_b = 0;
        std::vector<uint32_t> row_start;  // rows + 1 (dense)
        std::vector<uint32_t> entries;    // left offset | right offset << 16; width > 0, and always ahead of a list: [term][row], sign in bit 31
        std::vector<double> coeff;
        std::vector<uint32_t> row_map;    // per row: dense: image position << 16 | negate << 31 (the left_map word of the component the row produces); list: its element offset in the mid row
        std::vector<double> row_scale;    // per row (rescaled basis), else empty
        int left_len = 0, right_len = 0;
        int width = 0;                    // > 0: rows of one length with +-1 coefficients
    } pre;

    // PRODUCT_CSR (ELL form), list chain (plan_passes.cpp: chain_list_into_list): one operand of this list is the result of ANOTHER list
    // (`pre`) that nothing else reads -- (R X) ~R projected on a grade.  Both lists run in one k_product_ell_chain launch, the mid
    // row stays in LDS.
    struct Chain {
        int side = 0;                    // 1: the mid row is this list's left operand, 2: its right operand; 0: no chain
        int alias = 0;                   // this list's other operand: 0 = a row of its own, 1 = the first list's left row, 2 = its right row
        int mid_len = 0, canon_mid = 0, covered = 0;
        int ipb = 0, item_stride = 0, ent2_lds = 0;   // (bytes of this list's words kept in LDS, or 0)
    } chain;

    // ... specialised per program through hiprtc (plan_chain_jit.cpp: make_chain_jit; round 4): lane = (row, item) in BOTH lists with the items
    // of a workgroup fastest, so that the 32 lanes of an LDS access read one row's operand of 32 different items (odd item stride:
    // no bank conflict); entries carry byte offsets from the item's base (list 1: the sign is folded into a negated image of the
    // smaller operand); compile-time widths, lengths and strides.  The generic k_product_ell_chain stays as the fallback.
    struct ChainJit {
        int on = 0;                      // 1: source was generated (runtime.hip compiles it)
        std::string source;
        std::vector<uint32_t> ent1, pos1, ent2, out2;
        int single = 0;                  // the kernel runs a SINGLE list (few long rows): plan_passes.cpp: jit_long_row_lists
        int fold_prev = 0;               // ... and, once compiled, also the covering copy_grades_from step right before it
        BufRef init_src;                 // ... whose source gives the accumulators' starting values (pos1 = its offsets)
        int ipb = 0, threads = 0;
        size_t lds = 0;
        int split = 1;                            // slices per row of list 2 (> 1: re-ordered sums, tolerance mode; 1 with GAAST_FLAG_EXACT_ORDER)
        int xreg = 0;                             // tolerance mode: list 1's right operand in registers, its table re-ordered by right index (word: left offset | sign << 31)
        int sorted[3] = {0, 0, 0};               // tolerance mode, sign-sorted list 2: plus / minus terms per (row, slice), byte offset of the item's zero element
        int fmt[2] = {0, 0};                     // words per row of list 1's table; list 2's entries: 2 = wide (8 bytes: offsets, then the sign bit), 3 / 4 = sign-sorted clean words (LDS / global), else narrow
        int layout[7] = {0, 0, 0, 0, 0, 0, 0};   // an item in LDS, elements: offsets of l1, r1, the negated image, mid, r2 (-1: aliased); item stride; negated image is of the left operand
    } cj;

    // FUSED: the whole plan as one micro-op stream over per-item LDS slabs
    struct FusedInput {
        int slot, base, canon;
    };
    struct Fused {
        std::vector<uint32_t> prog;        // 32-word lines, see kernels.hip.hpp
        std::vector<uint32_t> phase_tab;   // per (phase, wave): first line, line count
        std::vector<double> general;       // the coefficients other than +-1 (passed by value)
        std::vector<FusedInput> inputs;
        int slab = 0, out_base = 0, zero_slot = 0;
        int jit_persistent = 0;   // > 0: the specialised kernel loops over groups (persistent workgroups): this many are resident per CU
        int jit_items = 0;        // items per workgroup of the specialised kernel when it is not one per thread (the slab-in-LDS form: 64)
        int jit_threads = 256;    // workgroup size of the specialised kernel (64: one wave per workgroup, coalesced row I/O through LDS)
        int jit_only = 0;         // the slab is too big for the LDS interpreter: runs only as the hiprtc-specialised kernel
        int jit_reg_trial = 0;    // one item per thread with a slab beyond 160 / 200 elements: kept only if the compiled kernel leaves two
                                  // waves per SIMD (runtime.hip: program_create_impl); else the plan is rebuilt with the slabs in LDS
        std::string jit_source;   // the plan as straight-line HIP (compiled with hiprtc at program_create)
    } fused;

    // EXPLOG (GAAST_FLAG_EXP_LOG extension): res += exp(arg) / log(arg), arg = buffer `a` holding a k-vector (log: + grade 0)
    struct ExpLog {
        int op = 0;                // 0 exp, 1 log
        int m = 0, mres = 0;       // components of the k-vector / of them that res holds (zip)
        int arg_k = 0, arg_0 = -1; // offsets in the operand row (grade k; grade 0 for log, -1 = absent)
        int res_k = -1, res_0 = -1;// offsets in the result row, -1 = not produced
        std::vector<double> sq;    // e_i e_i (blade squares, component order)
        // the domain check: pairs of distinct blades that commute, grouped by the blade T of their product in ascending T
        std::vector<uint32_t> row_start, pairs;   // pairs: i | j << 16
        std::vector<double> pair_coeff;           // 2 e_i e_j
    } explog;

    // EXPLOG_ADJ (GAAST_OP_EXP_ADJ / GAAST_OP_LOG_ADJ, gaast_hip.h): res += the cotangent of the exp / log operand, from the operand
    // row `a` (the k-vector B; log: + grade 0) and the row `b` holding the cotangent g of the forward result
    struct ExpLogAdj {
        int op = 0;                // 0 exp, 1 log
        int m = 0;                 // components of the k-vector
        int arg_k = 0, arg_0 = -1; // offsets in the operand row (grade k; grade 0 for log, -1 = absent)
        int g_k = -1, g_0 = -1;    // offsets in the cotangent row (grade k; exp: grade 0), -1 = absent (reads as 0)
        int mg = 0;                // grade-k components the cotangent row holds (zip with m): the ones the forward wrote
        int res_k = -1, res_0 = -1;// offsets in the result row (dB; log: da), -1 = not produced
        int mres = 0;              // grade-k components of dB that res holds (zip)
        std::vector<double> sq;    // e_i e_i (blade squares, component order)
    } adj;

    // DUAL (GAAST_OP_DUAL / GAAST_OP_UNDUAL, gaast_hip.h): res += the signed, grade-mirroring copy of row `a`.  One segment per source
    // grade, in ascending grade order: its `len` components are read at a_off, a_off + 1, ... and written at res_last, res_last - 1, ...
    // (component i of grade k goes to C(n,k) - 1 - i of grade n - k); bit t of `neg` negates the t-th component of the segments
    // laid end to end
    struct Dual {
        struct Seg { uint32_t a_off, res_last, len; };
        std::vector<Seg> segs;
        std::vector<uint32_t> neg;
        int total = 0;                  // components over all segments
        int undual = 0;                 // (the name only)
        template <typename F>
        void for_each(F&& f) const {    // f(result offset, operand offset, negate) in the order of the segments
            uint32_t t = 0;
            for (const Seg& g : segs)
                for (uint32_t i = 0; i < g.len; ++i, ++t) f(g.res_last - i, g.a_off + i, ((neg[t >> 5] >> (t & 31u)) & 1u) != 0);
        }
    } dual;

    // INVERSE (GAAST_OP_INV, gaast_hip.h): res += the Y with A Y = 1, A = row `a`.  The blade set S (every blade, or the even ones) in
    // ascending bitmask order: S[j] = j, or (j << 1) | parity(j) for the even set, so that the index of S[r] xor S[j] is r xor j.
    // Y solves L y = e_0 with L[r][j] = coeff(r, j) A[r xor j]: the matrix is held as what k_mv_inverse rebuilds it from -- the
    // reordering signs, one 64-bit word per row, and the metric factor by shared-vector set -- 4096 sign bits and at most 128 values
    struct Inverse {
        int N = 0;                          // |S|: 2, 4, ... 64
        int even = 0;                       // S is the even blades
        std::vector<uint32_t> blade;        // [N] the blade of index j
        std::vector<int32_t> a_off;         // [N] offset of blade j in the operand row; -1: the operand lacks its grade (reads as 0)
        std::vector<int32_t> res_off;       // [N] offset of blade j in the result row; -1: not produced
        uint64_t a_neg = 0;                 // bit j: the operand component is negated (sign-only arms over a bound input, folded)
        std::vector<uint64_t> neg;          // [N] bit j of neg[r]: e_a e_b = -(...) for a = S[r] xor S[j], b = S[j]
        std::vector<double> weight;         // [2^n] product of the metric diagonal over the vectors of the set s (a & b = S[j] & ~S[r])
        int n_out = 0;                      // produced components
        double coeff(int r, int j) const {  // L[r][j] = coeff(r, j) * A[r xor j]
            const double w = weight[size_t(blade[size_t(j)] & ~blade[size_t(r)])];
            return ((neg[size_t(r)] >> j) & 1ULL) ? -w : w;
        }
        // GEXP / GEXP_ADJ / GSQRT / GSQRT_ADJ / GLOG / GLOG_ADJ only (empty for INVERSE)
        double wmax = 1.0;                  // the largest |weight|: theta = wmax * sum |A_a| bounds the largest absolute row sum of L
        std::vector<int32_t> g_off;         // GEXP_ADJ, GSQRT_ADJ, GLOG_ADJ, GEXP_ADJ2, GLOG_ADJ2 [N] offset of blade j in the cotangent row; -1: absent (reads as 0)
        std::vector<int32_t> h_off;         // GEXP_JVP, GEXP_ADJ2, GSQRT_JVP, GLOG_JVP, GLOG_ADJ2 [N] offset of blade j in the tangent row (Step::c); -1: absent (reads as 0)
        // GEXP_ADJ: the sign words of the two adjoint products of P = X Z, both with the metric factor weight[S[a] & S[b]]:
        std::vector<uint64_t> adj_neg_l;    // [N] bit b of adj_neg_l[a] = bit b of neg[a xor b]:  ADJL(g, Z)[a] = sum_b +-w Z[b] g[a xor b]
        std::vector<uint64_t> adj_neg_r;    // [N] bit a of adj_neg_r[b] = bit b of neg[a xor b]:  ADJR(g, X)[b] = sum_a +-w X[a] g[a xor b]
        // GSQRT_JVP, GLOG_JVP, GLOG_ADJ2: the sign words of the (non-transposed) right-multiplication matrix R_M[r][j] = +-w M[r xor j], (u M)[r] = sum_j R_M[r][j] u[j],
        std::vector<uint64_t> rmul_neg;     // [N] bit j of rmul_neg[r]: e_a e_b = -(...) for a = S[j], b = S[r] xor S[j]; the metric factor is L's, weight[S[j] & ~S[r]]
    } inv;

    // GEXP (GAAST_OP_GEXP, gaast_hip.h): res += exp(A) by scaling and squaring, A = row `a`; the blade set and every table are INVERSE's
    // (`inv`, built by the same function: plan.cpp: blade_set_tables).  GEXP_ADJ (GAAST_OP_GEXP_ADJ): res += the cotangent of A from
    // A = row `a` and the cotangent g = row `b` of the forward result; inv.res_off then addresses the operand's grades in res.
    // GEXP_JVP (GAAST_OP_GEXP_JVP): res += the Frechet derivative of exp at A = row `a` in the direction h = row `c` (inv.h_off), in the
    // wanted grades of the blade set.  GEXP_ADJ2 (GAAST_OP_GEXP_ADJ2): res += the gradient in A of <g, GEXP_JVP(h, A)>, g = row `b`
    // (inv.g_off), h = row `c`; inv.res_off addresses the operand's grades in res.  Tables are GEXP_ADJ's; always launches of their own.
    // GSQRT (GAAST_OP_GSQRT, gaast_hip.h): res += the principal square root of A = row `a` by the Denman-Beavers product iteration, and
    // GSQRT_ADJ (GAAST_OP_GSQRT_ADJ): res += the cotangent of A, the solution of ADJL(a, X) + ADJR(a, X) = g.  Operands, blade set and
    // tables are GEXP's and GEXP_ADJ's, field for field (inv.wmax is not used; inv.adj_neg_l / adj_neg_r are the two sign words of a row of
    // the transposed L_X + R_X).  Like them the steps are always launches of their own.
    // GLOG (GAAST_OP_GLOG, gaast_hip.h): res += the principal logarithm of A = row `a` by inverse scaling and squaring (roots of GSQRT, a
    // [7/7] Pade approximant in partial fractions), and GLOG_ADJ (GAAST_OP_GLOG_ADJ): res += the cotangent of A.  Operands, blade set and
    // tables are GEXP's and GEXP_ADJ's again (inv.wmax scales the distance from e_0; inv.adj_neg_l is the sign word of a row of the
    // transposed R_M, inv.adj_neg_r of the transposed L_M).  Always launches of their own.
    // GSQRT_JVP / GLOG_JVP (GAAST_OP_GSQRT_JVP / GAAST_OP_GLOG_JVP): res += the tangent of the root / the logarithm at A = row `a` in the
    // direction h = row `c` (inv.h_off: any blades of the set), in the wanted grades of the blade set.  Tables are GSQRT's / GLOG's and
    // inv.rmul_neg; the rows of L_X + R_X, L_M and R_M all come from inv.neg, inv.rmul_neg and inv.weight.  Always launches of their own.
    // GLOG_ADJ2 (GAAST_OP_GLOG_ADJ2): res += the gradient in A of <g, GLOG_JVP(h, A)>, A = row `a`, g = row `b` (inv.g_off), h = row `c`
    // (inv.h_off), both any blades of the set; inv.res_off addresses the operand's grades in res.  It solves with the plain and the
    // transposed matrices, so it carries all four sign tables: inv.neg, inv.rmul_neg, inv.adj_neg_l, inv.adj_neg_r.  Always a launch of its own.

    // REDUCE_SCALE (plan_passes.cpp: fuse_reduce_scale): a product whose result is ONE scalar component (a single long row: norm_sq), an
    // optional ScalarUnaryOp on it, and a product of one-term rows that multiplies another row by that scalar -- the versor inverse
    // a.rev() * a.norm_sq().sinv() and normalisations, where the rows no longer fit a fused slab (n >= 9) -- in ONE launch, one wave per
    // item.  a / b = the reduction's operands.
    struct Reduce {
        std::vector<uint32_t> ent1;   // the reduction's terms in the reference's order: left | right << 16
        std::vector<double> coeff1;
        std::vector<uint32_t> ent2;   // the scaling's rows: operand offset | result offset << 16
        std::vector<double> coeff2;
        BufRef x;                     // the row that is scaled
        int canon_x = 0;
        int canon_s = 0;              // the scalar is re-read as a product operand: 0.0 + s
        int s_is_left = 0;            // the scalar is the scaling product's left operand
        int op = 0;                   // 0: none, 1: 1 / s, 2: sqrt(s)  (eval.rs:103-110)
        int wave = 0;                 // > 0: tolerance mode, the reduction is a signed sum of squares of the row that is scaled: 16-byte
                                      // pieces of the row per lane for k_reduce_scale_wave
        std::vector<uint32_t> sign_words;   // ... and the lanes' sign words
    } reduce;

    // ELEMENTWISE (plan_passes.cpp: fuse_elementwise_runs): a run of AXPY / FLIP steps on one buffer (and, when that buffer is only the operand
    // of a product of one-term rows with a scalar, that product too: the scaling epilogue) in one pass
    struct Elementwise {
        std::vector<BufRef> src;           // the source buffers
        std::vector<uint32_t> ops;         // [n_ops][n_comp] statement words
        std::vector<uint32_t> comp_off;    // the components' offsets in the run's buffer
        int n_ops = 0, load_first = 0;
        // with the scaling epilogue: b = the scalar operand (1-component row), res = the product's result
        int scale = 0, scalar_off = 0, canon_v = 0, canon_s = 0, s_is_left = 0;
        std::vector<uint32_t> out_off;     // result offsets
        std::vector<double> coeff;
    } ew;
    // LINMAP (gaast_hip_program_create_in_basis): res = the outermorphism of a change of basis applied to row buffer `a` -- an input
    // slot into the orthogonal basis of the program, or the root's result back into the caller's basis (kernels_linmap.hip.hpp)
};

// Every buffer a step reads, each given to f(BufRef): what the plan passes ask before they drop a buffer, what the runtime marks
// as used input slots.  (An absent operand has idx < 0.)
template <typename F>
void for_each_read(const Step& s, F&& f) {
    for (BufRef r : {s.a, s.b, s.c, s.pre.a, s.pre.b, s.reduce.x, s.cj.init_src})
        if (r.idx >= 0) f(r);
    for (BufRef r : s.ew.src) f(r);
    for (const Step::FusedInput& fi : s.fused.inputs) f(BufRef{BufKind::INPUT, fi.slot});
}
inline bool reads(const Step& s, BufRef buf) {
    bool hit = false;
    for_each_read(s, [&](BufRef r) { hit = hit || r == buf; });
    return hit;
}

// Launch-time forms of k_gp_mfma32p<false, 12, *, *>, as the dense launcher (runtime.hip: run_dense) derives them from the plan's
// maps; tests/cpp/dense_flags_driver.cpp checks them against the map words.
//   whole rows: every blade of the permuted basis has a place in the result row, no reordering sign, nothing accumulated, no rescaled
//   basis -- each result is one store at a lane-constant offset from the item's row;
//   signs per side: a side whose map words carry no sign bit is staged without the sign xor.
inline bool dense_whole_row_stores(const Step& s) { return s.dense.out_all && !s.dense.out_signs && !s.beta && !s.dense.scaled; }

// limits of this back end (gfx950): a product whose staged operands exceed the LDS of a CU, or whose comp-mul list
// exceeds the table budget, is valid in the reference but refused by gaast_hip_program_create (UNIMPLEMENTED)
constexpr size_t kLdsBytes = 160 * 1024;
#ifndef GAAST_INTERP_BUDGET_KB
#define GAAST_INTERP_BUDGET_KB 144   /* (build switch for A/B runs) */
#endif
constexpr size_t kInterpLdsBytes = size_t(GAAST_INTERP_BUDGET_KB) * 1024;   // slabs of the 64 items of a k_ast_fused workgroup
constexpr uint64_t kMaxListEntries = uint64_t(1) << 27;
constexpr uint64_t kMaxAdjointListEntries = uint64_t(1) << 22;   // compact adjoints regenerated as lists (n = 11 full: 4 M)

struct Plan {
    int n = 0;
    int dtype = GAAST_F64;
    uint32_t flags = 0;
    std::vector<double> metric;
    std::vector<gaast_input_desc> inputs;
    std::vector<std::vector<double>> const_rows;
    std::vector<Layout> input_layouts;
    std::vector<Layout> node_buffers;  // cache buffers other than the root's
    std::vector<char> node_dead;       // ... that no step touches any more, never allocated: the mid row of a chain (chain_sparse_into_dense,
                                       // chain_list_into_list), the buffer of an element-wise run with its scaling folded in
                                       // (fuse_elementwise_runs), the scalar of fuse_reduce_scale.  Sized by build_plan; plan_passes.cpp: mark_dead
                                       // is its only writer
    Layout out_layout;
    std::vector<Step> steps;
    int error = GAAST_OK;              // what the reference would have panicked with, at eval
    std::string error_msg;
    int has_explog = 0;                // some step evaluates exp / log: the program owns a domain-error counter
    int has_inverse = 0;               // some step is a general inverse: the program owns the domain-error counter too (singular items)
    int has_gexp = 0;                  // some step is a general exponential: it owns the domain-error counter too (theta out of range)
    int has_gsqrt = 0;                 // some step is a general square root: it owns the domain-error counter too (no principal root reached)
    int has_glog = 0;                  // some step is a general logarithm: it owns the domain-error counter too (no principal logarithm reached)
    int has_explog_adj = 0;            // some step is an exp / log adjoint (no interpreter micro-ops, no domain check)
    int mirrored = 0;                  // the program runs in the orthogonal basis of a Gram metric whose Q has det -1: every
                                       // complement sign and regressive coefficient is negated (gaast_hip.h: GAAST_OP_DUAL)
    std::string unsupported;           // non-empty: valid in the reference, beyond this back end (program_create fails)
    std::vector<char> slot_used;       // input slots some launch reads (the others may stay unbound)
    std::string jit_source_kept;       // GAAST_FLAG_DEBUG_KEEP_JIT_SOURCE
    // program in a non-orthonormal basis (gaast_hip_program_create_in_basis): the steps other than LINMAP read input slot i from
    // node buffer basis_slot_buf[i] (>= 0: its rows moved into the orthogonal basis) and write the root to node buffer basis_out_buf
    // (>= 0), which the last LINMAP step moves back into `out`
    std::vector<int> basis_slot_buf;
    int basis_out_buf = -1;

    const Layout& layout(BufRef r) const {   // the rows of a buffer a step names (r.idx >= 0)
        switch (r.kind) {
        case BufKind::NODE: return node_buffers[size_t(r.idx)];
        case BufKind::INPUT: return input_layouts[size_t(r.idx)];
        default: return out_layout;
        }
    }
};

// Throws std::runtime_error (-> GAAST_ERR_INVALID_PROGRAM) on malformed input.  small_reg_slab: the one-item-per-thread
// specialised kernel is limited to slabs of 160 / 200 elements (runtime.hip rebuilds a plan so when a bigger slab's trial
// compilation needs more than half of a SIMD's registers)
void build_plan(const gaast_program_desc& desc, Plan& plan, bool small_reg_slab = false, bool mirrored = false);

// Micro-op encoding shared by the plan builder and k_ast_fused (see kernels.hip.hpp).
namespace uop {
enum : uint32_t { LINE_MACS = 0, LINE_MISC = 1, LINE_NOP = 2, LINE_MACS_GEN = 3, LINE_MACS_CNT = 4, ADD = 3, NEG = 4, ZERO = 5, INV = 6, SQRT = 7, COPY = 8, SUB = 9, NCOPY = 10 };
constexpr int MAX_GENERAL_COEFFS = 6;
constexpr int MAX_INPUTS = 8;
constexpr int GROUPS = 8;  // waves per workgroup of k_ast_fused (FUSED_GROUPS)
}  // namespace uop

}  // namespace gaast
