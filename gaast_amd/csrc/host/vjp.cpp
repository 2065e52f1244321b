// Reverse mode: the vector-Jacobian product of a flat program as another flat program (gaast_program_vjp, gaast_expr.h).
//
// eval.rs evaluates in place: the root and every product operand get a buffer of their own (store_in_cache), and every other
// node adds into the buffer of the one that contains it (add_to_res).  A buffer is therefore built by a sequence of EVENTS --
// add an input, add a product, flip the sign of some grades (Negation / Reverse / GradeInvolution), apply a scalar op to grade 0
// (ScalarUnaryOp) -- and a flip or scalar op acts on everything accumulated before it, not only on its own child.  The adjoint
// walks each buffer's events backwards with the cotangent of that buffer:
//   input       the cotangent's grades of that input node go to the gradient (zip of the slice lengths, graded.rs:67-78);
//   product     transposed list -> cotangent of the operand buffers (explicit stays explicit, compact -> GAAST_PROD_ADJ_*);
//   flip        the same flip of the cotangent (kept as a per-grade sign and folded into the next list's coefficients);
//   SINV        t = 1/s: ds = -g t t;  SSQRT r = sqrt(s): ds = 0.5 g sinv(r) -- t and r are the buffer's grade 0 right after
//               the op, recomputed by a node that replays the buffer's events up to it;
//   dual/undual the operand has a buffer of its own or is read from a bound input (plan.cpp: lower_dual), so the node is a one-operand
//               product event: the operand's cotangent is the OTHER complement (the transpose of a signed permutation is its
//               inverse) of the buffer's cotangent restricted to the node's grades;
//   inv         (GAAST_OP_INV, gaast_hip.h) the operand has a buffer of its own or is read from a bound input (plan.cpp: lower_inverse):
//               a one-operand product event.  d(A^-1) = -(Y dA) Y with Y = A^-1, so the operand's cotangent is
//               -ADJ_RIGHT(ADJ_LEFT(g, Y), Y) over geometric products: Y is one more INV node over the forward operand that
//               produces every grade of its blade set, and the sign is a Negation of g -- of the innermost child, where it has a
//               buffer of its own (a product operand), so that every node added to a cotangent stays additive; by linearity the
//               bits are those of negating the result.  An INV node over a bare scalar (raw ABI) is a SINV event;
//   gexp        (GAAST_OP_GEXP, gaast_hip.h) the operand is read like inv's: a one-operand product event.  The operand's cotangent is one
//               GAAST_OP_GEXP_ADJ node over (the buffer's cotangent restricted to the node's grades, the forward operand): the
//               reverse sweep of the scaling-and-squaring recurrences, which recomputes the forward.  No flag;
//   gsqrt       (GAAST_OP_GSQRT, gaast_hip.h) like gexp: the operand's cotangent is one GAAST_OP_GSQRT_ADJ node over (the buffer's cotangent
//               restricted to the node's grades, the forward operand): the solve of ADJL(a, X) + ADJR(a, X) = g with the recomputed
//               root X.  No flag;
//   glog        (GAAST_OP_GLOG, gaast_hip.h) like gsqrt: the operand's cotangent is one GAAST_OP_GLOG_ADJ node over (the buffer's cotangent
//               restricted to the node's grades, the forward operand): the transposed Pade solves and the chain of root adjoints,
//               with the recomputed forward.  No flag;
//   exp / log   (GAAST_FLAG_EXP_LOG | GAAST_FLAG_EXP_LOG_GRAD) the operand has a buffer of its own, like a product operand
//               (plan.cpp: lower_exp_log -> store_in_cache): a one-operand product event -- GAAST_OP_EXP_ADJ / GAAST_OP_LOG_ADJ over
//               the buffer's cotangent restricted to the node's grades and the forward operand -> cotangent of the operand buffer.
// The function is closed under itself: a program it returned differentiates again.  Its explicit lists, NEG, INV, DUAL and PROJ
// nodes are forward nodes like any other; a compact GAAST_PROD_ADJ_* node is a product event whose operands' cotangents are, by the
// trilinear form <g, a o b> of the forward kind, the forward product or the other adjoint of the same kind (product_adjoint, table
// in gaast_expr.h); the adjoint op nodes (GAAST_OP_*_ADJ) are opaque events that are carried along off the path and refused by name
// on it (their derivative is a Frechet derivative of a matrix function) -- except, under GAAST_FLAG_GEXP_GRAD2, the family of the
// general exponential {GEXP_ADJ, GEXP_JVP, GEXP_ADJ2}, which has those kernels and is closed up to second order (gexp_family_adjoint),
// and, under GAAST_FLAG_GSQRT_GLOG_JVP, the families {GSQRT_ADJ, GSQRT_JVP}, closed at every order, and {GLOG_ADJ, GLOG_JVP}, closed with
// respect to child0 alone (root_log_family_adjoint) -- and, with GAAST_FLAG_GLOG_GRAD2 beside it, with respect to the operand too, up to
// second order, through GAAST_OP_GLOG_ADJ2.
// Buffers are visited from the root down (decreasing node index: a buffer's users come after it in post-order).  The adjoint
// program is evaluated in place as well, so every cotangent node it builds is ADDITIVE (input, product, or sums of them): adding
// it into a buffer adds its value.  Sign changes and projections of a cotangent that cannot be folded into a list are explicit
// products with a constant scalar 1 (slot n_inputs + 1).
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../common/algebra.hpp"
#include "../common/comp_mul_table.hpp"
#include "../common/grade_set.hpp"
#include "gaast_expr.h"

void gaast_set_expr_error(const std::string& msg);

namespace {

using namespace gaast;

struct VjpError {
    int status;
    std::string msg;
};

bool has_two_children(int opcode) {
    return opcode == GAAST_OP_ADD || opcode == GAAST_OP_PRODUCT || opcode == GAAST_OP_EXP_ADJ || opcode == GAAST_OP_LOG_ADJ || opcode == GAAST_OP_GEXP_ADJ || opcode == GAAST_OP_GSQRT_ADJ || opcode == GAAST_OP_GLOG_ADJ ||
           opcode == GAAST_OP_GEXP_JVP || opcode == GAAST_OP_GEXP_ADJ2 || opcode == GAAST_OP_GSQRT_JVP || opcode == GAAST_OP_GLOG_JVP ||
           opcode == GAAST_OP_GLOG_ADJ2;
}
// GAAST_OP_GEXP_ADJ2 and GAAST_OP_GLOG_ADJ2 have a third child, the forward operand: its node index travels in input_slot (gaast_hip.h); -1 for every other node
int third_child(const gaast_node_desc& nd) { return nd.opcode == GAAST_OP_GEXP_ADJ2 || nd.opcode == GAAST_OP_GLOG_ADJ2 ? nd.input_slot : -1; }

// the adjoint op nodes that gaast_program_vjp itself emits (child0 = a cotangent, child1 = the forward operand)
const char* adjoint_op_name(int opcode) {
    switch (opcode) {
    case GAAST_OP_EXP_ADJ: return "GAAST_OP_EXP_ADJ";
    case GAAST_OP_LOG_ADJ: return "GAAST_OP_LOG_ADJ";
    case GAAST_OP_GEXP_ADJ: return "GAAST_OP_GEXP_ADJ";
    case GAAST_OP_GSQRT_ADJ: return "GAAST_OP_GSQRT_ADJ";
    case GAAST_OP_GLOG_ADJ: return "GAAST_OP_GLOG_ADJ";
    case GAAST_OP_GEXP_JVP: return "GAAST_OP_GEXP_JVP";
    case GAAST_OP_GSQRT_JVP: return "GAAST_OP_GSQRT_JVP";
    case GAAST_OP_GLOG_JVP: return "GAAST_OP_GLOG_JVP";
    case GAAST_OP_GLOG_ADJ2: return "GAAST_OP_GLOG_ADJ2";
    default: return nullptr;
    }
}

enum EventKind { EV_INPUT, EV_PRODUCT, EV_FLIP, EV_SCALAR, EV_OPAQUE };
struct Event {
    EventKind kind;
    int node;
    std::vector<std::pair<int, int>> path;  // (ancestor, which child) from the buffer's node down to `node`
};

// cotangent of a buffer = sum over terms of flip_sigma(proj_kappa(value of node))
struct Term {
    int node;
    uint64_t sigma;  // grades whose sign is flipped
    uint64_t kappa;  // grades kept
};

struct Builder {
    const gaast_program_desc& d;
    const int wrt;
    const int n;
    std::vector<gaast_node_desc> nodes;
    std::vector<std::vector<gaast_comp_mul>> lists;  // owned explicit lists (forward nodes keep their pointers)
    std::vector<char> dep;                           // forward node depends on input `wrt`
    int one_node = -1, cot_node = -1;
    double one_value = 1.0;

    Builder(const gaast_program_desc& desc, int slot) : d(desc), wrt(slot), n(desc.vec_space_dim) {}

    int add(gaast_node_desc nd, std::vector<gaast_comp_mul> list = {}) {
        nodes.push_back(nd);
        lists.push_back(std::move(list));
        return int(nodes.size()) - 1;
    }
    gaast_node_desc blank(int opcode, uint64_t mask, int dim) const {
        gaast_node_desc nd{};
        nd.opcode = opcode;
        nd.child0 = nd.child1 = -1;
        nd.minimal_grade_mask = mask;
        nd.vec_space_dim = dim;
        nd.input_slot = -1;
        nd.product_kind = GAAST_PROD_EXPLICIT;
        return nd;
    }
    int one() {
        if (one_node < 0) {
            gaast_node_desc nd = blank(GAAST_OP_INPUT, 1ULL, n);
            nd.input_slot = d.n_inputs + 1;
            one_node = add(nd);
        }
        return one_node;
    }
    int explicit_product(int c0, int c1, std::vector<gaast_comp_mul> list, uint64_t mask, int dim) {
        gaast_node_desc nd = blank(GAAST_OP_PRODUCT, mask, dim);
        nd.child0 = c0;
        nd.child1 = c1;
        nd.n_comp_muls = list.size();
        return add(nd, std::move(list));
    }
    // sum of additive nodes (ADD chain); -1 for none
    int sum(const std::vector<int>& parts, uint64_t mask, int dim) {
        if (parts.empty()) return -1;
        int acc = parts[0];
        for (size_t i = 1; i < parts.size(); ++i) {
            gaast_node_desc nd = blank(GAAST_OP_ADD, mask, dim);
            nd.child0 = acc;
            nd.child1 = parts[i];
            acc = add(nd);
        }
        return acc;
    }
    uint64_t mask_of(int i) const { return nodes[size_t(i)].minimal_grade_mask; }

    // copy of grades `want` of a term, signs applied, as (component) x 1 -> (component); slices zipped to `dim`
    std::vector<gaast_comp_mul> copy_list(const Term& t, uint64_t want, int dim) const {
        std::vector<gaast_comp_mul> list;
        const int tn = nodes[size_t(t.node)].vec_space_dim;
        for (int k = 0; k < 64; ++k) {
            if (!((want >> k) & 1ULL)) continue;
            const uint64_t len = std::min(n_choose_k(uint64_t(tn), uint64_t(k)), n_choose_k(uint64_t(dim), uint64_t(k)));
            for (uint64_t i = 0; i < len; ++i)
                list.push_back(gaast_comp_mul{uint32_t(k), uint32_t(i), 0, 0, uint32_t(k), uint32_t(i),
                                              ((t.sigma >> k) & 1ULL) ? -1.0 : 1.0});
        }
        return list;
    }
    // the value of a cotangent restricted to `mask`, as one additive node whose minimal mask is within `mask`; -1 when zero
    int materialize(const std::vector<Term>& terms, uint64_t mask) {
        if (terms.size() == 1) {
            const Term& t = terms[0];
            const uint64_t m = mask_of(t.node);
            if ((m & ~mask) == 0 && (m & ~t.kappa) == 0 && (m & t.sigma) == 0 && nodes[size_t(t.node)].vec_space_dim == n)
                return t.node;
        }
        std::vector<int> parts;
        for (const Term& t : terms) {
            const uint64_t want = mask_of(t.node) & t.kappa & mask;
            if (want) parts.push_back(explicit_product(t.node, one(), copy_list(t, want, n), mask, n));
        }
        return sum(parts, mask, n);
    }

    void collect(int x, std::vector<std::pair<int, int>>& path, std::vector<Event>& ev) const {
        const gaast_node_desc& nd = d.nodes[x];
        if (nd.minimal_grade_mask == 0) return;  // eval.rs:40-43
        switch (nd.opcode) {
        case GAAST_OP_INPUT: ev.push_back({EV_INPUT, x, path}); return;
        case GAAST_OP_PRODUCT: ev.push_back({EV_PRODUCT, x, path}); return;
        case GAAST_OP_ADD:
            path.push_back({x, 0});
            collect(nd.child0, path, ev);
            path.back().second = 1;
            collect(nd.child1, path, ev);
            path.pop_back();
            return;
        case GAAST_OP_NEG:
        case GAAST_OP_REVERSE:
        case GAAST_OP_GINVOL:
        case GAAST_OP_SINV:
        case GAAST_OP_SSQRT:
        case GAAST_OP_PROJ:
            path.push_back({x, 0});
            collect(nd.child0, path, ev);
            path.pop_back();
            if (nd.opcode == GAAST_OP_SINV || nd.opcode == GAAST_OP_SSQRT) ev.push_back({EV_SCALAR, x, path});
            else if (nd.opcode != GAAST_OP_PROJ) ev.push_back({EV_FLIP, x, path});
            return;
        case GAAST_OP_INV:
            if (d.nodes[nd.child0].minimal_grade_mask == 1ULL) {  // of a bare scalar: lowered as ScalarInversion
                path.push_back({x, 0});
                collect(nd.child0, path, ev);
                path.pop_back();
                ev.push_back({EV_SCALAR, x, path});
                return;
            }
            ev.push_back({EV_OPAQUE, x, path});
            return;
        default: ev.push_back({EV_OPAQUE, x, path}); return;  // exp / log, dual / undual, gexp, gsqrt, glog and the adjoint op nodes
        }
    }
    // inv: cotangent of the operand's buffer
    void inv_adjoint(int x, const std::vector<Term>& terms, std::vector<std::vector<Term>>& cot) {
        const gaast_node_desc& xd = d.nodes[x];
        const int c = xd.child0;
        if (!dep[size_t(c)]) return;
        const uint64_t cmask = d.nodes[c].minimal_grade_mask, smask = gs_inverse(cmask, n);
        const int g = materialize(terms, xd.minimal_grade_mask);
        if (g < 0 || !cmask) return;
        gaast_node_desc y = blank(GAAST_OP_INV, smask, n);
        y.child0 = c;
        const int yn = add(y);
        gaast_node_desc neg = blank(GAAST_OP_NEG, mask_of(g), n);
        neg.child0 = g;
        const int ng = add(neg);
        const Selection sel{GAAST_PROD_GEOMETRIC, nullptr, nullptr, n};
        gaast_node_desc m = blank(GAAST_OP_PRODUCT, smask, n);   // cotangent of M = Y dA in P = M Y
        m.child0 = ng;
        m.child1 = yn;
        m.product_kind = GAAST_PROD_GEOMETRIC + GAAST_PROD_ADJ_LEFT;
        m.n_comp_muls = comp_mul_count(n, iter_contribs(mask_of(ng), sel, smask, smask));
        const int mn = add(m);
        gaast_node_desc a = blank(GAAST_OP_PRODUCT, cmask, n);   // cotangent of dA in M = Y dA
        a.child0 = mn;
        a.child1 = yn;
        a.product_kind = GAAST_PROD_GEOMETRIC + GAAST_PROD_ADJ_RIGHT;
        a.n_comp_muls = comp_mul_count(n, iter_contribs(smask, sel, smask, cmask));
        cot[size_t(c)].push_back(Term{add(a), 0, ~0ULL});
    }
    // gexp: cotangent of the operand's buffer (gaast_hip.h: GAAST_OP_GEXP_ADJ)
    void gexp_adjoint(int x, const std::vector<Term>& terms, std::vector<std::vector<Term>>& cot) {
        const gaast_node_desc& xd = d.nodes[x];
        const int c = xd.child0;
        if (!dep[size_t(c)]) return;
        const uint64_t cmask = d.nodes[c].minimal_grade_mask;
        const int g = materialize(terms, xd.minimal_grade_mask);
        if (g < 0 || !cmask) return;
        gaast_node_desc nd = blank(GAAST_OP_GEXP_ADJ, cmask, n);
        nd.child0 = g;
        nd.child1 = c;
        cot[size_t(c)].push_back(Term{add(nd), 0, ~0ULL});
    }
    // GAAST_FLAG_GEXP_GRAD2: the cotangents of the operands of a GEXP_ADJ / GEXP_JVP node x (table in gaast_expr.h).  Both are bilinear
    // in (child0, the Frechet derivative at A): <k, GEXP_ADJ(g, A)> = <g, GEXP_JVP(k, A)>, whose gradient in A is GEXP_ADJ2(g, k, A)
    void gexp_family_adjoint(int x, const std::vector<Term>& terms, std::vector<std::vector<Term>>& cot) {
        const gaast_node_desc& xd = d.nodes[x];
        if (xd.opcode == GAAST_OP_GEXP_ADJ2)
            throw VjpError{GAAST_ERR_UNIMPLEMENTED, "third-order reverse mode through GAAST_OP_GEXP_ADJ2 is not implemented"};
        const bool jvp = xd.opcode == GAAST_OP_GEXP_JVP;
        const int c0 = xd.child0, a = xd.child1;
        const uint64_t amask = d.nodes[a].minimal_grade_mask, c0mask = d.nodes[c0].minimal_grade_mask;
        if (!dep[size_t(c0)] && !dep[size_t(a)]) return;
        const int k = materialize(terms, xd.minimal_grade_mask);
        if (k < 0 || !amask) return;
        if (dep[size_t(c0)] && c0mask) {   // linear in child0: the transposed map at the same A
            gaast_node_desc nd = blank(jvp ? GAAST_OP_GEXP_ADJ : GAAST_OP_GEXP_JVP, c0mask, n);
            nd.child0 = k;
            nd.child1 = a;
            cot[size_t(c0)].push_back(Term{add(nd), 0, ~0ULL});
        }
        if (dep[size_t(a)] && c0mask) {
            gaast_node_desc nd = blank(GAAST_OP_GEXP_ADJ2, amask, n);
            nd.child0 = jvp ? k : c0;    // g
            nd.child1 = jvp ? c0 : k;    // h
            nd.input_slot = a;
            cot[size_t(a)].push_back(Term{add(nd), 0, ~0ULL});
        }
    }
    // gsqrt: cotangent of the operand's buffer (gaast_hip.h: GAAST_OP_GSQRT_ADJ)
    void gsqrt_adjoint(int x, const std::vector<Term>& terms, std::vector<std::vector<Term>>& cot) {
        const gaast_node_desc& xd = d.nodes[x];
        const int c = xd.child0;
        if (!dep[size_t(c)]) return;
        const uint64_t cmask = d.nodes[c].minimal_grade_mask;
        const int g = materialize(terms, xd.minimal_grade_mask);
        if (g < 0 || !cmask) return;
        gaast_node_desc nd = blank(GAAST_OP_GSQRT_ADJ, cmask, n);
        nd.child0 = g;
        nd.child1 = c;
        cot[size_t(c)].push_back(Term{add(nd), 0, ~0ULL});
    }
    // glog: cotangent of the operand's buffer (gaast_hip.h: GAAST_OP_GLOG_ADJ)
    void glog_adjoint(int x, const std::vector<Term>& terms, std::vector<std::vector<Term>>& cot) {
        const gaast_node_desc& xd = d.nodes[x];
        const int c = xd.child0;
        if (!dep[size_t(c)]) return;
        const uint64_t cmask = d.nodes[c].minimal_grade_mask;
        const int g = materialize(terms, xd.minimal_grade_mask);
        if (g < 0 || !cmask) return;
        gaast_node_desc nd = blank(GAAST_OP_GLOG_ADJ, cmask, n);
        nd.child0 = g;
        nd.child1 = c;
        cot[size_t(c)].push_back(Term{add(nd), 0, ~0ULL});
    }
    // GAAST_FLAG_GSQRT_GLOG_JVP: the cotangents of the operands of a GSQRT_ADJ / GSQRT_JVP / GLOG_ADJ / GLOG_JVP node x (table in
    // gaast_expr.h).  Each is linear in child0, the tangent map at A or its transpose, so child0's cotangent is the other node of the pair
    // over (k, A).  For gsqrt the map is S^-1 with S = L_X + R_X, X the root of A:  d(S^-1) = -S^-1 (L_dX + R_dX) S^-1 and dX = S^-1 dA
    // give the gradient in A of <g, S^-1 h> as -GSQRT_ADJ(ADJ_LEFT(w, u) + ADJ_RIGHT(w, u), A) over geometric products, with
    // w = GSQRT_ADJ(g, A) and u = GSQRT_JVP(h, A) on every grade of the blade set.  The sign is a Negation of k, the innermost child,
    // as inv_adjoint places it and for its reason.  For glog the gradient in A needs GAAST_FLAG_GLOG_GRAD2 as well and is one
    // GAAST_OP_GLOG_ADJ2 node over (g, h, A), the two vectors of the pair in that order; a GLOG_ADJ2 node on the path is refused.
    void root_log_family_adjoint(int x, const std::vector<Term>& terms, std::vector<std::vector<Term>>& cot) {
        const gaast_node_desc& xd = d.nodes[x];
        const bool log = xd.opcode == GAAST_OP_GLOG_ADJ || xd.opcode == GAAST_OP_GLOG_JVP;
        const bool jvp = xd.opcode == GAAST_OP_GSQRT_JVP || xd.opcode == GAAST_OP_GLOG_JVP;
        const int op_adj = log ? GAAST_OP_GLOG_ADJ : GAAST_OP_GSQRT_ADJ, op_jvp = log ? GAAST_OP_GLOG_JVP : GAAST_OP_GSQRT_JVP;
        const int c0 = xd.child0, a = xd.child1;
        if (xd.opcode == GAAST_OP_GLOG_ADJ2)
            throw VjpError{GAAST_ERR_UNIMPLEMENTED, "third-order reverse mode through GAAST_OP_GLOG_ADJ2 is not implemented"};
        const bool grad2 = (d.flags & GAAST_FLAG_GSQRT_GLOG_JVP) && (d.flags & GAAST_FLAG_GLOG_GRAD2);
        if (log && dep[size_t(a)] && !grad2)
            throw VjpError{GAAST_ERR_UNIMPLEMENTED, std::string("reverse mode through ") + adjoint_op_name(xd.opcode) + " with respect to its operand is not implemented"};
        const uint64_t amask = d.nodes[a].minimal_grade_mask, c0mask = d.nodes[c0].minimal_grade_mask;
        if (!dep[size_t(c0)] && !dep[size_t(a)]) return;
        const int k = materialize(terms, xd.minimal_grade_mask);
        if (k < 0 || !amask || !c0mask) return;
        if (dep[size_t(c0)]) {   // linear in child0: the transposed map at the same A
            gaast_node_desc nd = blank(jvp ? op_adj : op_jvp, c0mask, n);
            nd.child0 = k;
            nd.child1 = a;
            cot[size_t(c0)].push_back(Term{add(nd), 0, ~0ULL});
        }
        if (dep[size_t(a)] && log) {   // GAAST_FLAG_GLOG_GRAD2: bilinear in (g, h) at A, one node (gaast_hip.h: GAAST_OP_GLOG_ADJ2)
            gaast_node_desc nd = blank(GAAST_OP_GLOG_ADJ2, amask, n);
            nd.child0 = jvp ? k : c0;    // g
            nd.child1 = jvp ? c0 : k;    // h
            nd.input_slot = a;
            cot[size_t(a)].push_back(Term{add(nd), 0, ~0ULL});
        } else if (dep[size_t(a)]) {
            const uint64_t smask = gs_inverse(amask, n);
            gaast_node_desc neg = blank(GAAST_OP_NEG, mask_of(k), n);
            neg.child0 = k;
            const int nk = add(neg);
            gaast_node_desc w = blank(GAAST_OP_GSQRT_ADJ, smask, n);   // w = S^-T g
            w.child0 = jvp ? nk : c0;
            w.child1 = a;
            const int wn = add(w);
            gaast_node_desc u = blank(GAAST_OP_GSQRT_JVP, smask, n);   // u = S^-1 h
            u.child0 = jvp ? c0 : nk;
            u.child1 = a;
            const int un = add(u);
            const Selection sel{GAAST_PROD_GEOMETRIC, nullptr, nullptr, n};
            gaast_node_desc l = blank(GAAST_OP_PRODUCT, smask, n);    // cotangent of dX in dX u
            l.child0 = wn;
            l.child1 = un;
            l.product_kind = GAAST_PROD_GEOMETRIC + GAAST_PROD_ADJ_LEFT;
            l.n_comp_muls = comp_mul_count(n, iter_contribs(smask, sel, smask, smask));
            gaast_node_desc r = l;                                    // cotangent of dX in u dX
            r.product_kind = GAAST_PROD_GEOMETRIC + GAAST_PROD_ADJ_RIGHT;
            const int ln = add(l), rn = add(r);
            gaast_node_desc out = blank(GAAST_OP_GSQRT_ADJ, amask, n);
            out.child0 = sum({ln, rn}, smask, n);
            out.child1 = a;
            cot[size_t(a)].push_back(Term{add(out), 0, ~0ULL});
        }
    }
    // dual / undual: cotangent of the operand's buffer
    void dual_adjoint(int x, const std::vector<Term>& terms, std::vector<std::vector<Term>>& cot) {
        const gaast_node_desc& xd = d.nodes[x];
        const int c = xd.child0;
        if (!dep[size_t(c)]) return;
        const uint64_t cmask = d.nodes[c].minimal_grade_mask & gs_mirror(xd.minimal_grade_mask, n);
        const int g = materialize(terms, xd.minimal_grade_mask);
        if (g < 0 || !cmask) return;
        gaast_node_desc nd = blank(xd.opcode == GAAST_OP_DUAL ? GAAST_OP_UNDUAL : GAAST_OP_DUAL, cmask, n);
        nd.child0 = g;
        cot[size_t(c)].push_back(Term{add(nd), 0, ~0ULL});
    }
    // exp / log: cotangent of the operand's buffer (gaast_hip.h: GAAST_OP_EXP_ADJ / GAAST_OP_LOG_ADJ)
    void explog_adjoint(int x, const std::vector<Term>& terms, std::vector<std::vector<Term>>& cot) {
        const gaast_node_desc& xd = d.nodes[x];
        const int c = xd.child0;
        if ((d.flags & (GAAST_FLAG_EXP_LOG | GAAST_FLAG_EXP_LOG_GRAD)) != (GAAST_FLAG_EXP_LOG | GAAST_FLAG_EXP_LOG_GRAD))
            throw VjpError{GAAST_ERR_UNIMPLEMENTED, "exp / log on the path to the differentiated input has no adjoint"};
        if (!dep[size_t(c)]) return;
        const uint64_t cmask = d.nodes[c].minimal_grade_mask;
        if (xd.opcode == GAAST_OP_EXP && cmask == 1ULL)
            throw VjpError{GAAST_ERR_UNIMPLEMENTED, "exp of a bare scalar on the path to the differentiated input has no adjoint"};
        const int g = materialize(terms, xd.minimal_grade_mask);
        if (g < 0) return;
        gaast_node_desc nd = blank(xd.opcode == GAAST_OP_EXP ? GAAST_OP_EXP_ADJ : GAAST_OP_LOG_ADJ, cmask, n);
        nd.child0 = g;
        nd.child1 = c;
        cot[size_t(c)].push_back(Term{add(nd), 0, ~0ULL});
    }
    static uint64_t flip_set(const gaast_node_desc& nd) {
        const uint64_t gs = nd.minimal_grade_mask;
        if (nd.opcode == GAAST_OP_NEG) return gs;
        uint64_t m = 0;
        for (int k = 0; k < 64; ++k) {
            if (!((gs >> k) & 1ULL)) continue;
            if (nd.opcode == GAAST_OP_REVERSE ? (k % 4 == 2 || k % 4 == 3) : (k & 1)) m |= 1ULL << k;
        }
        return m;
    }
    // a node whose evaluation into a fresh buffer of buffer node s replays s's events up to and including event e
    int replay(int s, const Event& e) {
        const uint64_t ms = d.nodes[s].minimal_grade_mask;
        int prefix = e.node;
        for (size_t i = e.path.size(); i-- > 0;) {
            const gaast_node_desc& a = d.nodes[e.path[i].first];
            if (a.opcode == GAAST_OP_ADD && e.path[i].second == 1) {  // the left sibling's events came first
                gaast_node_desc nd = blank(GAAST_OP_ADD, ms, n);
                nd.child0 = a.child0;
                nd.child1 = prefix;
                prefix = add(nd);
            }
        }
        gaast_node_desc nd = blank(GAAST_OP_PROJ, ms, n);
        nd.child0 = prefix;
        return add(nd);
    }

    // cotangent of a product's operand buffer, from the cotangent of the buffer the product adds into
    void product_adjoint(int p, const std::vector<Term>& terms, std::vector<std::vector<Term>>& cot) {
        const gaast_node_desc& pd = d.nodes[p];
        for (int side = 0; side < 2; ++side) {
            const int c = side ? pd.child1 : pd.child0, other = side ? pd.child0 : pd.child1;
            if (!dep[size_t(c)]) continue;
            const uint64_t cmask = d.nodes[c].minimal_grade_mask;
            // a geometric product from n = 6 on keeps its adjoint compact even when the forward list is explicit: the plan can then
            // run it on the dense kernels (the list it would regenerate is the very same, product_kind names it)
            if (pd.comp_muls && !(pd.product_kind == GAAST_PROD_GEOMETRIC && n >= 6)) {
                for (const Term& t : terms) {
                    const uint64_t avail = mask_of(t.node) & t.kappa;
                    std::vector<gaast_comp_mul> fwd;
                    fwd.reserve(size_t(pd.n_comp_muls));
                    for (uint64_t e = 0; e < pd.n_comp_muls; ++e) {
                        gaast_comp_mul m = pd.comp_muls[e];
                        if (m.result_grade >= 64 || !((avail >> m.result_grade) & 1ULL)) continue;
                        if ((t.sigma >> m.result_grade) & 1ULL) m.coeff = -m.coeff;
                        fwd.push_back(m);
                    }
                    if (fwd.empty()) continue;
                    auto adj = transpose_comp_muls(fwd.data(), fwd.size(), side == 1, false);
                    const int node = side ? explicit_product(other, t.node, std::move(adj), cmask, n)
                                          : explicit_product(t.node, other, std::move(adj), cmask, n);
                    // the entries of a regressive list are pseudoscalar-valued: an explicit list that names the kind gets the
                    // orientation sign of a Gram basis at lowering (gaast_hip.h: GAAST_PROD_REGRESSIVE), and so must its transpose
                    if (pd.product_kind == GAAST_PROD_REGRESSIVE) nodes[size_t(node)].product_kind = GAAST_PROD_REGRESSIVE;
                    cot[size_t(c)].push_back(Term{node, 0, ~0ULL});
                }
            } else {
                const int adj = pd.product_kind >= 0 ? (pd.product_kind & ~7) : 0, base = pd.product_kind & 7;
                if (pd.product_kind < 0 || base > GAAST_PROD_REGRESSIVE || (adj && adj != GAAST_PROD_ADJ_LEFT && adj != GAAST_PROD_ADJ_RIGHT))
                    throw VjpError{GAAST_ERR_INVALID_PROGRAM, "PRODUCT node has neither a comp-mul list nor a product kind"};
                const int g = materialize(terms, pd.minimal_grade_mask);
                if (g < 0) continue;
                gaast_node_desc nd = blank(GAAST_OP_PRODUCT, cmask, n);
                const Selection sel{base, nullptr, nullptr, n};
                const bool regressive = base == GAAST_PROD_REGRESSIVE;
                if (!adj) {
                    nd.child0 = g;
                    nd.child1 = other;
                    nd.product_kind = pd.product_kind + (side ? GAAST_PROD_ADJ_RIGHT : GAAST_PROD_ADJ_LEFT);
                    const uint64_t lmask = side ? mask_of(other) : cmask, rmask = side ? cmask : mask_of(other);
                    nd.n_comp_muls = comp_mul_count(n, iter_contribs(mask_of(g), sel, lmask, rmask), regressive);
                } else if (side == 0) {
                    // a compact adjoint node P = ADJ(g0, x) is <h, P> = T(g0, h, x) (ADJ_LEFT) or T(g0, x, h) (ADJ_RIGHT) with the
                    // trilinear form T(g, a, b) = <g, a o b> of the forward kind and h = g here, the cotangent of P.  For g0, the
                    // forward product of the other two in their forward order
                    nd.child0 = adj == GAAST_PROD_ADJ_LEFT ? g : other;
                    nd.child1 = adj == GAAST_PROD_ADJ_LEFT ? other : g;
                    nd.product_kind = base;
                    nd.n_comp_muls = comp_mul_count(n, iter_contribs(cmask, sel, mask_of(nd.child0), mask_of(nd.child1)), regressive);
                } else {
                    // for x, the adjoint of the other side over (g0, h)
                    nd.child0 = other;
                    nd.child1 = g;
                    nd.product_kind = base + (adj == GAAST_PROD_ADJ_LEFT ? GAAST_PROD_ADJ_RIGHT : GAAST_PROD_ADJ_LEFT);
                    const uint64_t lmask = adj == GAAST_PROD_ADJ_LEFT ? mask_of(g) : cmask, rmask = adj == GAAST_PROD_ADJ_LEFT ? cmask : mask_of(g);
                    nd.n_comp_muls = comp_mul_count(n, iter_contribs(mask_of(other), sel, lmask, rmask), regressive);
                }
                cot[size_t(c)].push_back(Term{add(nd), 0, ~0ULL});
            }
        }
    }

    void scalar_adjoint(int s, const Event& e, std::vector<Term>& terms) {
        const gaast_node_desc& x = d.nodes[e.node];
        const int t = replay(s, e);
        int factor = t;          // SINV: -g t t
        double c = -1.0;
        if (x.opcode == GAAST_OP_SSQRT) {  // 0.5 g sinv(r)
            gaast_node_desc nd = blank(GAAST_OP_SINV, d.nodes[s].minimal_grade_mask, n);
            nd.child0 = t;
            factor = add(nd);
            c = 0.5;
        }
        std::vector<int> parts;
        for (Term& term : terms) {
            if ((mask_of(term.node) & term.kappa) & 1ULL) {
                const double sg = (term.sigma & 1ULL) ? -c : c;
                parts.push_back(explicit_product(term.node, factor, {gaast_comp_mul{0, 0, 0, 0, 0, 0, sg}}, 1ULL, n));
            }
            term.kappa &= ~1ULL;
        }
        int ds = sum(parts, 1ULL, n);
        if (ds < 0) return;
        if (x.opcode != GAAST_OP_SSQRT) ds = explicit_product(ds, t, {gaast_comp_mul{0, 0, 0, 0, 0, 0, 1.0}}, 1ULL, n);
        terms.push_back(Term{ds, 0, ~0ULL});
    }

    int build() {
        const int nf = d.n_nodes;
        const gaast_input_desc& in = d.inputs[wrt];
        const int sd = in.storage_dim;
        for (int i = 0; i < nf; ++i) add(d.nodes[i]);
        dep.assign(size_t(nf), 0);
        for (int i = 0; i < nf; ++i) {
            const gaast_node_desc& nd = d.nodes[i];
            if (nd.opcode == GAAST_OP_INPUT) dep[size_t(i)] = nd.input_slot == wrt;
            else dep[size_t(i)] = dep[size_t(nd.child0)] || (nd.child1 >= 0 && has_two_children(nd.opcode) && dep[size_t(nd.child1)]) ||
                                  (third_child(nd) >= 0 && dep[size_t(third_child(nd))]);
        }
        std::vector<std::vector<Term>> cot(static_cast<size_t>(nf));
        std::vector<int> outs;
        if (dep[size_t(d.root)] && d.nodes[d.root].minimal_grade_mask) {
            gaast_node_desc nd = blank(GAAST_OP_INPUT, d.nodes[d.root].minimal_grade_mask, n);
            nd.input_slot = d.n_inputs;
            cot_node = add(nd);
            cot[size_t(d.root)].push_back(Term{cot_node, 0, ~0ULL});
        }
        for (int s = d.root; s >= 0; --s) {
            if (cot[size_t(s)].empty()) continue;
            std::vector<Term> terms = std::move(cot[size_t(s)]);
            std::vector<Event> ev;
            std::vector<std::pair<int, int>> path;
            collect(s, path, ev);
            std::vector<char> dep_upto(ev.size(), 0);
            for (size_t i = 0; i < ev.size(); ++i) {
                const bool self = (ev[i].kind == EV_INPUT || ev[i].kind == EV_PRODUCT || ev[i].kind == EV_OPAQUE) && dep[size_t(ev[i].node)];
                dep_upto[i] = char(self || (i > 0 && dep_upto[i - 1]));
            }
            for (size_t i = ev.size(); i-- > 0;) {
                if (!dep_upto[i]) break;  // nothing before this point reaches input `wrt`
                const Event& e = ev[i];
                const gaast_node_desc& x = d.nodes[e.node];
                switch (e.kind) {
                case EV_INPUT: {
                    if (x.input_slot != wrt) break;
                    const uint64_t used = x.minimal_grade_mask & in.grade_mask;
                    for (const Term& t : terms) {
                        const uint64_t m = mask_of(t.node), want = m & t.kappa & used;
                        if (!want) continue;
                        if ((m & ~want) == 0 && (m & t.sigma) == 0 && sd == n && nodes[size_t(t.node)].vec_space_dim == n)
                            outs.push_back(t.node);
                        else
                            outs.push_back(explicit_product(t.node, one(), copy_list(t, want, sd), in.grade_mask, sd));
                    }
                    break;
                }
                case EV_PRODUCT: product_adjoint(e.node, terms, cot); break;
                case EV_FLIP: {
                    const uint64_t f = flip_set(x);
                    for (Term& t : terms) t.sigma ^= f;
                    break;
                }
                case EV_SCALAR: scalar_adjoint(s, e, terms); break;
                case EV_OPAQUE:   // a node whose operand has a buffer of its own
                    if ((d.flags & GAAST_FLAG_GEXP_GRAD2) && (x.opcode == GAAST_OP_GEXP_ADJ || x.opcode == GAAST_OP_GEXP_JVP)) {
                        gexp_family_adjoint(e.node, terms, cot);   // (the family is closed up to second order)
                    } else if ((d.flags & GAAST_FLAG_GSQRT_GLOG_JVP) && (x.opcode == GAAST_OP_GSQRT_ADJ || x.opcode == GAAST_OP_GSQRT_JVP ||
                                                                          x.opcode == GAAST_OP_GLOG_ADJ || x.opcode == GAAST_OP_GLOG_JVP)) {
                        root_log_family_adjoint(e.node, terms, cot);   // (gsqrt: closed at every order; glog: with respect to child0)
                    } else if (x.opcode == GAAST_OP_GEXP_ADJ2) {
                        if (dep[size_t(e.node)]) gexp_family_adjoint(e.node, terms, cot);   // (refused, with or without the flag)
                    } else if (x.opcode == GAAST_OP_GLOG_ADJ2) {
                        if (dep[size_t(e.node)]) root_log_family_adjoint(e.node, terms, cot);   // (refused, with or without the flags)
                    } else if (const char* name = adjoint_op_name(x.opcode)) {   // its second derivative needs a Frechet-derivative kernel
                        if (dep[size_t(e.node)])
                            throw VjpError{GAAST_ERR_UNIMPLEMENTED, std::string("second-order reverse mode through ") + name + " is not implemented"};
                    } else if (x.opcode == GAAST_OP_DUAL || x.opcode == GAAST_OP_UNDUAL) dual_adjoint(e.node, terms, cot);
                    else if (x.opcode == GAAST_OP_INV) inv_adjoint(e.node, terms, cot);
                    else if (x.opcode == GAAST_OP_GEXP) gexp_adjoint(e.node, terms, cot);
                    else if (x.opcode == GAAST_OP_GSQRT) gsqrt_adjoint(e.node, terms, cot);
                    else if (x.opcode == GAAST_OP_GLOG) glog_adjoint(e.node, terms, cot);
                    else explog_adjoint(e.node, terms, cot);
                    break;
                }
            }
        }
        int root;
        if (outs.empty()) {  // the input does not reach the root: zero rows (one product that adds 0 * 1 * 1)
            int k0 = 0;
            while (k0 < 63 && !((in.grade_mask >> k0) & 1ULL)) ++k0;
            const int o = one();
            gaast_node_desc nd = blank(GAAST_OP_PROJ, 0, sd);
            nd.child0 = o;
            root = in.grade_mask ? explicit_product(o, o, {gaast_comp_mul{0, 0, 0, 0, uint32_t(k0), 0, 0.0}}, in.grade_mask, sd) : add(nd);
        } else if (outs.size() == 1) {
            gaast_node_desc nd = blank(GAAST_OP_PROJ, in.grade_mask, sd);
            nd.child0 = outs[0];
            root = (mask_of(outs[0]) == in.grade_mask && nodes[size_t(outs[0])].vec_space_dim == sd) ? outs[0] : add(nd);
        } else {
            root = sum(outs, in.grade_mask, sd);
        }
        return root;
    }
};

}  // namespace

extern "C" int gaast_program_vjp(const gaast_program_desc* desc, int32_t wrt_slot, gaast_program_image_t* out) {
    if (!desc || !out) {
        gaast_set_expr_error("null argument");
        return GAAST_ERR_INVALID_ARGUMENT;
    }
    *out = nullptr;
    const gaast_program_desc& d = *desc;
    if (d.n_nodes <= 0 || !d.nodes || d.root < 0 || d.root >= d.n_nodes || d.n_inputs < 0 || d.n_inputs > GAAST_MAX_INPUTS ||
        (d.n_inputs && !d.inputs) || d.vec_space_dim < 0 || d.vec_space_dim > GAAST_MAX_DIM) {
        gaast_set_expr_error("malformed program description");
        return GAAST_ERR_INVALID_PROGRAM;
    }
    if (wrt_slot < 0 || wrt_slot >= d.n_inputs || d.inputs[wrt_slot].is_const) {
        gaast_set_expr_error("wrt_slot is out of range or names a const input");
        return GAAST_ERR_INVALID_ARGUMENT;
    }
    if (d.n_inputs + 1 > GAAST_MAX_INPUTS) {
        gaast_set_expr_error("no input slot is left for the cotangent");
        return GAAST_ERR_INVALID_ARGUMENT;
    }
    if (d.flags & GAAST_FLAG_SPINOR_GEMM) {
        gaast_set_expr_error("GAAST_FLAG_SPINOR_GEMM programs have no VJP");
        return GAAST_ERR_UNIMPLEMENTED;
    }
    for (int i = 0; i < d.n_nodes; ++i) {
        const gaast_node_desc& nd = d.nodes[i];
        const bool two = has_two_children(nd.opcode);
        const bool ok = nd.opcode == GAAST_OP_INPUT ? (nd.input_slot >= 0 && nd.input_slot < d.n_inputs)
                        : (nd.opcode > GAAST_OP_INPUT && nd.opcode <= GAAST_OP_GLOG_ADJ2 &&
                           nd.child0 >= 0 && nd.child0 < i &&
                           (!two || (nd.child1 >= 0 && nd.child1 < i)) &&
                           ((nd.opcode != GAAST_OP_GEXP_ADJ2 && nd.opcode != GAAST_OP_GLOG_ADJ2) || (nd.input_slot >= 0 && nd.input_slot < i)));
        // a compact adjoint product (a VJP program differentiates again): GAAST_PROD_ADJ_LEFT or GAAST_PROD_ADJ_RIGHT over a kind 0..5
        const int adj = nd.product_kind & ~7, base = nd.product_kind & 7;
        const bool kind_ok = nd.opcode != GAAST_OP_PRODUCT || nd.product_kind < GAAST_PROD_ADJ_LEFT ||
                             ((adj == GAAST_PROD_ADJ_LEFT || adj == GAAST_PROD_ADJ_RIGHT) && base <= GAAST_PROD_REGRESSIVE);
        if (!ok || !kind_ok) {
            gaast_set_expr_error("malformed program description (node " + std::to_string(i) + ")");
            return GAAST_ERR_INVALID_PROGRAM;
        }
    }
    try {
        Builder b(d, wrt_slot);
        const int root = b.build();
        if (b.one_node >= 0 && d.n_inputs + 2 > GAAST_MAX_INPUTS) {
            gaast_set_expr_error("no input slot is left for the constant 1 of the adjoint");
            return GAAST_ERR_INVALID_ARGUMENT;
        }
        // keep what the root reaches, in post-order
        std::vector<int> keep(b.nodes.size(), 0), remap(b.nodes.size(), -1);
        keep[size_t(root)] = 1;
        for (size_t i = b.nodes.size(); i-- > 0;) {
            if (!keep[i]) continue;
            const gaast_node_desc& nd = b.nodes[i];
            if (nd.child0 >= 0) keep[size_t(nd.child0)] = 1;
            if (nd.child1 >= 0 && has_two_children(nd.opcode)) keep[size_t(nd.child1)] = 1;
            if (third_child(nd) >= 0) keep[size_t(third_child(nd))] = 1;
        }
        std::vector<gaast_node_desc> nodes;
        for (size_t i = 0; i < b.nodes.size(); ++i) {
            if (!keep[i]) continue;
            gaast_node_desc nd = b.nodes[i];
            if (nd.child0 >= 0) nd.child0 = remap[size_t(nd.child0)];
            if (nd.child1 >= 0) nd.child1 = has_two_children(nd.opcode) ? remap[size_t(nd.child1)] : -1;
            if (third_child(nd) >= 0) nd.input_slot = remap[size_t(nd.input_slot)];
            if (nd.opcode == GAAST_OP_PRODUCT && i >= size_t(d.n_nodes) && !b.lists[i].empty())   // (explicit; a regressive one names its kind)
                nd.comp_muls = b.lists[i].data();
            remap[i] = int(nodes.size());
            nodes.push_back(nd);
        }
        std::vector<gaast_input_desc> inputs(d.inputs, d.inputs + d.n_inputs);
        inputs.push_back(gaast_input_desc{d.nodes[d.root].minimal_grade_mask, d.vec_space_dim, 0, nullptr});
        if (b.one_node >= 0 && keep[size_t(b.one_node)]) inputs.push_back(gaast_input_desc{1ULL, 0, 1, &b.one_value});
        gaast_program_desc a = d;
        a.n_nodes = int(nodes.size());
        a.nodes = nodes.data();
        a.root = remap[size_t(root)];
        a.n_inputs = int(inputs.size());
        a.inputs = inputs.data();
        // the image owns copies of every array: round trip through the wire format
        const size_t len = gaast_program_serialize(&a, nullptr, 0);
        std::vector<unsigned char> buf(len);
        gaast_program_serialize(&a, buf.data(), len);
        *out = gaast_program_deserialize(buf.data(), len);
        if (!*out) {
            gaast_set_expr_error("adjoint program could not be encoded");
            return GAAST_ERR_INVALID_PROGRAM;
        }
        return GAAST_OK;
    } catch (const VjpError& e) {
        gaast_set_expr_error(e.msg);
        return e.status;
    } catch (const std::exception& e) {
        gaast_set_expr_error(e.what());
        return GAAST_ERR_INVALID_PROGRAM;
    }
}
