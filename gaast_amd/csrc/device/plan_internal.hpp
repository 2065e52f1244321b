// What the translation units of the plan builder share (device/plan*.cpp: plan.cpp, plan_dense.cpp, plan_fused.cpp,
// plan_chain_jit.cpp, plan_passes.cpp); not part of plan.hpp's interface.
#pragma once
#include <map>
#include <utility>

#include "plan.hpp"

namespace gaast {

// plan_fused.cpp.  Whole-plan fusion for small programs: replaces the plan's steps with one FUSED step (true), or changes nothing.
bool try_fuse(Plan& plan, bool small_reg_slab);
// ... the slab size that fused plan would have; 0: the plan cannot be fused
int fused_slab(const Plan& plan, bool small_reg_slab);

// plan_chain_jit.cpp.  The list chain of step `c` (second list) and `wp` (first list) as a hiprtc-specialised kernel: fills c.cj, or
// leaves c.cj.on = 0.  wp == nullptr: a single list; init_off: the offsets of the covering copy folded into it.
void make_chain_jit(const Plan& plan, Step& c, const Step* wp, int64_t l1, int64_t r1, int64_t mid, int64_t r2, int alias, int side, bool covered,
                    const std::vector<uint32_t>* init_off = nullptr);

// plan_passes.cpp.  The whole-plan rewrites of a lowered plan that was not fused whole, in this order: fuse_elementwise_runs,
// fuse_reduce_scale, chain_sparse_into_dense, uniform_csr_to_ell, chain_list_into_list, jit_long_row_lists.
void run_plan_passes(Plan& plan);
// ... two of them, which build_plan also tries on their own (a program that is exactly one list chain)
void uniform_csr_to_ell(Plan& plan);
void chain_list_into_list(Plan& plan);

// The state of the walk over the program (plan.cpp: struct Lowering derives from it) that the product paths of plan_dense.cpp work on.
struct LowerState {
    const gaast_program_desc& d;
    Plan& plan;
    BladeTable bt;
    std::map<std::pair<int, int>, int> fresh;  // buffer -> index of its still-untouched ZERO step
    std::vector<char> removed;                 // per emitted step: dropped when the walk ends (a zero fill folded into its first writer)

    LowerState(const gaast_program_desc& desc, Plan& p) : d(desc), plan(p), bt(desc.vec_space_dim) {}

    const gaast_node_desc& node(int i) const { return d.nodes[i]; }
    const Layout& layout(BufRef r) const { return plan.layout(r); }
    static std::pair<int, int> key(BufRef r) { return {int(r.kind), r.idx}; }
    void touch(BufRef r) { fresh.erase(key(r)); }

    bool fail(int status, const std::string& msg) {
        if (plan.error == GAAST_OK) {
            plan.error = status;
            plan.error_msg = msg;
        }
        return false;
    }
    bool ok() const { return plan.error == GAAST_OK; }

    Step& emit(Step::Kind k, BufRef res, const std::string& name) {
        plan.steps.emplace_back();
        removed.push_back(0);
        Step& s = plan.steps.back();
        s.kind = k;
        s.res = res;
        s.name = name;
        return s;
    }
};

// What lower_product (plan.cpp) has resolved when it hands a Product node to one of its three paths
struct ProductOperands {
    const gaast_node_desc& nd;
    BufRef res, l, r;               // result; left and right operand rows (operand(): a bound input in place, or its cache buffer)
    int canon_l, canon_r;           // ... read as 0.0 + x
    uint64_t flip_l, flip_r;        // grades of the operand that sign-only arms over the input negate
    uint64_t lmin, rmin;            // minimal grade sets of the two child nodes
    int fresh_zero;                 // >= 0: res is untouched and its zero fill -- this step -- may be folded into the product
};

// plan_dense.cpp.  The algebra a dense kernel runs in: the program's (n, metric), or -- for a product of parity-pure operands -- the
// even subalgebra Cl+(p, q) = Cl(n - 1) built on a pivot vector e_p (plan_dense.cpp: parity_reduced_frame).
struct DenseFrame {
    int n = 0;
    std::vector<double> metric;
    int pivot = -1;            // >= 0: parity-reduced; the basis vector of the program's algebra the reduction is built on
    int lpar = -1, rpar = -1;  // parity of the left / right operand (0 even, 1 odd) when reduced
};
// which dense kernel family takes a product, in which algebra (frame) and in which basis of it (position j of the permuted basis
// holds vector perm[j] of the frame's)
struct DenseChoice {
    DenseFamily family = DenseFamily::VECTOR_FMA;
    DenseFrame frame;
    std::vector<int> perm;
};
// does a dense kernel take the product (then `c` says which and how) / do the opt-in matrix-representation kernels?
bool dense_choice(const LowerState& st, const ProductOperands& po, DenseChoice& c);
bool spinor_eligible(const LowerState& st, const ProductOperands& po);
// one PRODUCT_DENSE step each; the result buffer holds every grade the product produces (lower_product has checked)
void lower_product_dense(LowerState& st, const ProductOperands& po, const DenseChoice& c);
void lower_product_spinor(LowerState& st, const ProductOperands& po);

}  // namespace gaast
