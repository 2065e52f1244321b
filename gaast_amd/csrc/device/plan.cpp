// Lowering of a flat SpecializedAst program into kernel launches.  See plan.hpp.
//
// The walk below IS the reference's interpreter (src/eval.rs) with every data-touching
// statement replaced by "emit a launch":
//   store_in_cache  eval.rs:21-33     add_to_res  eval.rs:35-115
// Three exact rewrites are applied unless GAAST_FLAG_NO_FUSION is set:
//   (1) a Product operand that is a bound input holding every wanted grade is read in place
//       (the kernel applies the `0.0 + x` of the reference's zero-init + add_grades_from copy,
//       eval.rs:27-31 / graded.rs:74) instead of being copied to a cache buffer;
//   (2) a Product that is the first writer of a fresh buffer starts its sums from the
//       zero-initialised accumulator in registers and the zero-fill launch is dropped;
//   (3) products whose list is a dense slice of the geometric product's table run on the
//       bitmask-tiled kernel (re-ordered sums: tolerance, not bit-exact; GAAST_FLAG_EXACT_ORDER
//       keeps them on the exact kernel).
#include "plan_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>

namespace gaast {
namespace {

struct Lowering : LowerState {
    std::vector<int> cache;               // node -> node_buffers index, -1 = not cached

    Lowering(const gaast_program_desc& desc, Plan& p) : LowerState(desc, p), cache(size_t(desc.n_nodes), -1) {}

    void emit_zero(BufRef buf) {
        emit(Step::ZERO, buf, "zero_fill[init_null_mv]");
        fresh[key(buf)] = int(plan.steps.size()) - 1;
    }

    // eval.rs:21-33
    BufRef store_in_cache(int id) {
        if (cache[size_t(id)] >= 0) return BufRef{BufKind::NODE, cache[size_t(id)]};
        plan.node_buffers.push_back(make_layout(node(id).vec_space_dim, node(id).minimal_grade_mask));
        const int b = int(plan.node_buffers.size()) - 1;
        cache[size_t(id)] = b;
        BufRef buf{BufKind::NODE, b};
        emit_zero(buf);
        add_to_res(buf, id);
        return buf;
    }

    // every offset of the grades of `mask` inside `res`; MISSING_GRADE if res lacks one
    bool offsets_of(BufRef res, uint64_t mask, std::vector<uint32_t>& out) {
        const Layout& l = layout(res);
        for (int k = 0; k < 64; ++k) {
            if (!((mask >> k) & 1ULL)) continue;
            if (!((l.mask >> k) & 1ULL))
                return fail(GAAST_ERR_MISSING_GRADE, "grade " + std::to_string(k) + " absent from result buffer");
            for (int64_t i = 0; i < l.grade_len(k); ++i) out.push_back(uint32_t(l.offset(k) + i));
        }
        return true;
    }

    void emit_flip(BufRef res, uint64_t mask, const char* what) {
        std::vector<uint32_t> offs;
        if (!offsets_of(res, mask, offs)) return;
        if (offs.empty()) return;
        Step& s = emit(Step::FLIP, res, std::string("negate_grades[") + what + "]");
        s.flip_offsets = std::move(offs);
        touch(res);
    }

    // can the operand be read straight from the bound input?
    bool direct_input_ok(int id) const {
        const gaast_node_desc& nd = node(id);
        if (nd.opcode != GAAST_OP_INPUT) return false;
        const Layout& in = plan.input_layouts[size_t(nd.input_slot)];
        const uint64_t want = nd.minimal_grade_mask;
        if ((in.mask & want) != want) return false;  // a wanted grade would stay zero in the copy
        for (int k = 0; k < 64; ++k)
            if (((want >> k) & 1ULL) && in.grade_len(k) != int64_t(n_choose_k(uint64_t(nd.vec_space_dim), uint64_t(k))))
                return false;                         // zip() would truncate (graded.rs:73)
        return true;
    }

    // eval.rs:35-115
    void add_to_res(BufRef res, int id) {
        if (!ok()) return;
        const gaast_node_desc& nd = node(id);
        const uint64_t gs = nd.minimal_grade_mask;
        if (gs == 0) return;  // eval.rs:40-43
        switch (nd.opcode) {
        case GAAST_OP_INPUT: {  // eval.rs:45-50 -> graded.rs:67-78
            const Layout& in = plan.input_layouts[size_t(nd.input_slot)];
            const Layout& r = layout(res);
            std::vector<uint32_t> map;
            for (int k = 0; k < 64; ++k) {
                if (!((gs >> k) & 1ULL) || !((in.mask >> k) & 1ULL)) continue;
                if (!((r.mask >> k) & 1ULL)) {
                    fail(GAAST_ERR_MISSING_GRADE, "grade " + std::to_string(k) + " absent from result buffer");
                    return;
                }
                const int64_t len = std::min(r.grade_len(k), in.grade_len(k));  // zip
                for (int64_t i = 0; i < len; ++i)
                    map.push_back(uint32_t(r.offset(k) + i) | (uint32_t(in.offset(k) + i) << 16));
            }
            if (map.empty()) return;
            // the first writer of a fresh buffer that covers every component of it: the zero fill is folded into the copy
            // (res = 0.0 + in: init_null_mv then `*r = *r + i`, graded.rs:74) -- one launch and one pass over res less
            const auto fr = fresh.find(key(res));
            const bool covers = fr != fresh.end() && !(plan.flags & GAAST_FLAG_NO_FUSION) && int64_t(map.size()) == r.row_len;
            if (covers) removed[size_t(fr->second)] = 1;
            Step& s = emit(Step::AXPY, res, std::string(covers ? "copy_grades_from" : "add_grades_from") + "[input " + std::to_string(nd.input_slot) + "]");
            s.a = BufRef{BufKind::INPUT, nd.input_slot};
            s.axpy_map = std::move(map);
            s.beta = covers ? 0 : 1;
            touch(res);
            return;
        }
        case GAAST_OP_ADD:  // eval.rs:51-54
            add_to_res(res, nd.child0);
            add_to_res(res, nd.child1);
            return;
        case GAAST_OP_NEG:  // eval.rs:55-60
            add_to_res(res, nd.child0);
            if (ok()) emit_flip(res, gs, "Negation");
            return;
        case GAAST_OP_REVERSE: {  // eval.rs:87-94
            add_to_res(res, nd.child0);
            if (!ok()) return;
            if ((gs & 1ULL) && (plan.flags & GAAST_FLAG_DEBUG_OVERFLOW)) {
                fail(GAAST_ERR_OVERFLOW, "attempt to subtract with overflow (Reverse over grade 0, debug build)");
                return;
            }
            uint64_t m = 0;
            for (int k = 0; k < 64; ++k)
                if (((gs >> k) & 1ULL) && (k % 4 == 2 || k % 4 == 3)) m |= 1ULL << k;  // (k(k-1)/2) odd
            emit_flip(res, m, "Reverse");
            return;
        }
        case GAAST_OP_GINVOL: {  // eval.rs:95-102
            add_to_res(res, nd.child0);
            if (!ok()) return;
            uint64_t m = 0;
            for (int k = 1; k < 64; k += 2)
                if ((gs >> k) & 1ULL) m |= 1ULL << k;
            emit_flip(res, m, "GradeInvolution");
            return;
        }
        case GAAST_OP_SINV:
        case GAAST_OP_SSQRT: {  // eval.rs:103-110
            add_to_res(res, nd.child0);
            if (!ok()) return;
            const Layout& r = layout(res);
            if (!(r.mask & 1ULL)) {
                fail(GAAST_ERR_MISSING_GRADE, "scalar op on a buffer without grade 0");
                return;
            }
            Step& s = emit(Step::SUNARY, res, nd.opcode == GAAST_OP_SINV ? "scalar_inversion" : "scalar_sqrt");
            s.sunary_op = nd.opcode == GAAST_OP_SINV ? 0 : 1;
            s.sunary_off = int(r.offset(0));
            touch(res);
            return;
        }
        case GAAST_OP_PROJ: add_to_res(res, nd.child0); return;  // eval.rs:111
        case GAAST_OP_EXP:
        case GAAST_OP_LOG:  // eval.rs:112-113
            if (plan.flags & GAAST_FLAG_EXP_LOG) {
                lower_exp_log(res, id);
                return;
            }
            fail(GAAST_ERR_UNIMPLEMENTED, "Exponential / Logarithm evaluation is todo!() in the reference");
            return;
        case GAAST_OP_EXP_ADJ:
        case GAAST_OP_LOG_ADJ: lower_exp_log_adj(res, id); return;
        case GAAST_OP_DUAL:
        case GAAST_OP_UNDUAL: lower_dual(res, id); return;
        case GAAST_OP_INV: lower_inverse(res, id); return;
        case GAAST_OP_GEXP: lower_gexp(res, id, Step::GEXP, "gexp", "the general exponential", "general_exponential"); return;
        case GAAST_OP_GEXP_ADJ: lower_gexp_adj(res, id, Step::GEXP_ADJ, "gexp", "the general exponential's adjoint", "general_exponential_adjoint"); return;
        case GAAST_OP_GEXP_JVP:
        case GAAST_OP_GEXP_ADJ2: lower_gexp2(res, id); return;
        case GAAST_OP_GSQRT: lower_gexp(res, id, Step::GSQRT, "gsqrt", "the general square root", "general_sqrt"); return;
        case GAAST_OP_GSQRT_ADJ: lower_gexp_adj(res, id, Step::GSQRT_ADJ, "gsqrt", "the general square root's adjoint", "general_sqrt_adjoint"); return;
        case GAAST_OP_GLOG: lower_gexp(res, id, Step::GLOG, "glog", "the general logarithm", "general_log"); return;
        case GAAST_OP_GLOG_ADJ: lower_gexp_adj(res, id, Step::GLOG_ADJ, "glog", "the general logarithm's adjoint", "general_log_adjoint"); return;
        case GAAST_OP_GSQRT_JVP: lower_root_log_jvp(res, id, Step::GSQRT_JVP, "gsqrt", "the general square root's tangent", "general_sqrt_jvp"); return;
        case GAAST_OP_GLOG_JVP: lower_root_log_jvp(res, id, Step::GLOG_JVP, "glog", "the general logarithm's tangent", "general_log_jvp"); return;
        case GAAST_OP_GLOG_ADJ2: lower_glog_adj2(res, id); return;
        case GAAST_OP_PRODUCT: lower_product(res, id); return;
        default: throw std::runtime_error("unknown opcode");
        }
    }

    // Complements (GAAST_OP_DUAL / GAAST_OP_UNDUAL, gaast_hip.h; no reference counterpart): a one-operand product arm.  The operand is
    // read like a Product's (operand(): a bound input in place, sign-only arms over it folded into the signs, else its cache buffer,
    // eval.rs:67-68); res += +-x, component i of grade k at component C(n,k) - 1 - i of grade n - k.
    void lower_dual(BufRef res, int id) {
        const gaast_node_desc& nd = node(id);
        const int n = d.vec_space_dim;
        const bool undual = nd.opcode == GAAST_OP_UNDUAL;
        const uint64_t want = gs_mirror(nd.minimal_grade_mask, n) & node(nd.child0).minimal_grade_mask;   // source grades
        if (!want) return;
        int canon = 0;
        uint64_t flip = 0;
        BufRef a = operand(nd.child0, &canon, &flip);
        if (!ok()) return;
        if (key(a) == key(res)) {
            fail(GAAST_ERR_MISSING_GRADE, "complement operand aliases its own result buffer");
            return;
        }
        const Layout &la = layout(a), &lr = layout(res);
        Step::Dual q;
        q.undual = undual;
        const uint64_t full = (uint64_t(1) << n) - 1;
        for (int k = 0; k <= n; ++k) {
            if (!((want >> k) & 1ULL) || !((la.mask >> k) & 1ULL)) continue;
            if (!((lr.mask >> (n - k)) & 1ULL)) {
                fail(GAAST_ERR_MISSING_GRADE, "grade " + std::to_string(n - k) + " absent from result buffer");
                return;
            }
            const int64_t c = int64_t(bt.grade_dim[size_t(k)]);
            if (lr.grade_len(n - k) != c) throw std::runtime_error("complement into a buffer of another dimension");
            const int64_t len = std::min(la.grade_len(k), c);   // (an operand stored in a smaller dimension: its leading components)
            if (len <= 0) continue;
            q.segs.push_back({uint32_t(la.offset(k)), uint32_t(lr.offset(n - k) + c - 1), uint32_t(len)});
            for (int64_t i = 0; i < len; ++i) {
                const uint64_t s = bt.blade_of[size_t(k)][size_t(i)];
                const int neg = (complement_parity(n, undual ? (~s & full) : s) + int((flip >> k) & 1ULL) + plan.mirrored) & 1;
                if ((q.total & 31) == 0) q.neg.push_back(0u);
                if (neg) q.neg.back() |= 1u << (q.total & 31);
                ++q.total;
            }
        }
        if (!q.total) return;
        // the first writer of a fresh buffer that covers every component of it: the zero fill is folded in (res = 0.0 + (+-x))
        const auto fr = fresh.find(key(res));
        const bool covers = fr != fresh.end() && !(plan.flags & GAAST_FLAG_NO_FUSION) && int64_t(q.total) == lr.row_len;
        if (covers) removed[size_t(fr->second)] = 1;
        Step& s = emit(Step::DUAL, res, std::string(undual ? "undual" : "dual") + "[" + std::to_string(q.total) + " components, n=" + std::to_string(n) + "]");
        s.a = a;
        s.canon_a = canon;
        s.beta = covers ? 0 : 1;
        s.dual = std::move(q);
        touch(res);
    }

    // The tables of a step over the blade set S (Step::Inverse: INVERSE, GEXP, GEXP_ADJ, GEXP_JVP, GEXP_ADJ2, GSQRT, GSQRT_ADJ, GSQRT_JVP, GLOG, GLOG_ADJ, GLOG_JVP, GLOG_ADJ2): S itself, where operand row `a` (grades
    // `amask`, those of `flip` negated) and result row `res` (grades `produce`) hold its blades, the reordering signs and the metric
    // factors of the left-multiplication matrix.  false: failed (a produced grade is absent from res)
    bool blade_set_tables(Step::Inverse& q, bool even, BufRef a, uint64_t amask, uint64_t flip, BufRef res, uint64_t produce) {
        const int n = d.vec_space_dim;
        const Layout &la = layout(a), &lr = layout(res);
        q.even = even ? 1 : 0;
        q.N = 1 << (even ? n - 1 : n);
        q.weight.assign(size_t(1) << n, 1.0);
        for (uint32_t sset = 0; sset < (uint32_t(1) << n); ++sset)
            for (int bit = 0; bit < n; ++bit)   // ascending bit order, as blades_gp_coeff multiplies
                if ((sset >> bit) & 1u) q.weight[sset] *= d.metric_diag[bit];
        for (int j = 0; j < q.N; ++j) {
            const uint32_t b = even ? (uint32_t(j) << 1) | uint32_t(__builtin_popcount(uint32_t(j)) & 1) : uint32_t(j);
            const int k = __builtin_popcount(b);
            q.blade.push_back(b);
            const bool held = ((amask >> k) & 1ULL) && ((la.mask >> k) & 1ULL) && int64_t(bt.index_of[b]) < la.grade_len(k);
            q.a_off.push_back(held ? int32_t(la.offset(k) + bt.index_of[b]) : -1);
            if (held && ((flip >> k) & 1ULL)) q.a_neg |= uint64_t(1) << j;
            int32_t ro = -1;
            if ((produce >> k) & 1ULL) {
                if (!((lr.mask >> k) & 1ULL) || lr.grade_len(k) != int64_t(bt.grade_dim[size_t(k)])) {
                    fail(GAAST_ERR_MISSING_GRADE, "grade " + std::to_string(k) + " absent from result buffer");
                    return false;
                }
                ro = int32_t(lr.offset(k) + bt.index_of[b]);
                ++q.n_out;
            }
            q.res_off.push_back(ro);
        }
        q.neg.assign(size_t(q.N), 0);
        for (int r = 0; r < q.N; ++r)
            for (int j = 0; j < q.N; ++j)
                if (reorder_parity(q.blade[size_t(r)] ^ q.blade[size_t(j)], q.blade[size_t(j)])) q.neg[size_t(r)] |= uint64_t(1) << j;
        return true;
    }

    // is a general exponential, square root or logarithm over this blade set beyond the kernels (N = 2 ... 64)?  Then the plan is marked unsupported
    bool blade_set_unsupported(const char* what, bool even) {
        const int n = d.vec_space_dim, bits = even ? n - 1 : n;
        if (bits >= 1 && bits <= 6) return false;
        if (plan.unsupported.empty())
            plan.unsupported = std::string(what) + " over " + (even ? "the even blades" : "every blade") + " of a " + std::to_string(n) +
                               "-dimensional algebra: the kernel is built for 2 to 64 blades";
        return true;
    }

    // The general exponential (GAAST_OP_GEXP, gaast_hip.h; no reference counterpart): a one-operand product arm, always a launch of
    // its own (Step::GEXP, k_mv_gexp).  The operand is read like the inverse's; res += exp(A) in the wanted grades.  The general square
    // root (GAAST_OP_GSQRT; Step::GSQRT, k_mv_gsqrt) is lowered by the same lines: `kind` the step's, `op` / `what` / `label` its names
    // in messages and in the launch name.  So is the general logarithm (GAAST_OP_GLOG; Step::GLOG, k_mv_glog).
    void lower_gexp(BufRef res, int id, Step::Kind kind, const std::string& op, const char* what, const char* label) {
        const gaast_node_desc& nd = node(id);
        const gaast_node_desc& ch = node(nd.child0);
        const int n = d.vec_space_dim;
        if (ch.vec_space_dim != n || nd.vec_space_dim != n) {
            fail(GAAST_ERR_INVALID_PROGRAM, op + " operand lives in another vector space than the algebra");
            return;
        }
        const uint64_t amask = ch.minimal_grade_mask & ((uint64_t(2) << n) - 1);
        const bool even = !(amask & 0xAAAAAAAAAAAAAAAAULL);
        if (blade_set_unsupported(what, even)) return;
        int canon = 0;
        uint64_t flip = 0;
        BufRef a = operand(nd.child0, &canon, &flip);
        if (!ok()) return;
        if (key(a) == key(res)) {
            fail(GAAST_ERR_MISSING_GRADE, op + " operand aliases its own result buffer");
            return;
        }
        const Layout& lr = layout(res);
        Step::Inverse q;
        if (!blade_set_tables(q, even, a, amask, flip, res, nd.minimal_grade_mask)) return;
        q.wmax = 0.0;
        for (double w : q.weight) q.wmax = std::max(q.wmax, std::fabs(w));
        if (!q.n_out) return;
        // the first writer of a fresh buffer that covers every component of it: the zero fill is folded in
        const auto fr = fresh.find(key(res));
        const bool covers = fr != fresh.end() && !(plan.flags & GAAST_FLAG_NO_FUSION) && int64_t(q.n_out) == lr.row_len;
        if (covers) removed[size_t(fr->second)] = 1;
        Step& s = emit(kind, res, std::string(label) + "[" + std::to_string(q.N) + (even ? " even" : "") + " blades, " + std::to_string(q.n_out) + " produced, n=" + std::to_string(n) + "]");
        s.a = a;
        s.canon_a = canon;
        s.beta = covers ? 0 : 1;
        s.inv = std::move(q);
        (kind == Step::GLOG ? plan.has_glog : kind == Step::GSQRT ? plan.has_gsqrt : plan.has_gexp) = 1;
        touch(res);
    }

    // [N] where row layout `l` holds the blades of the set; -1: absent (a cotangent or tangent row: read as 0)
    std::vector<int32_t> blade_offsets(const Step::Inverse& q, const Layout& l) const {
        std::vector<int32_t> off;
        for (int j = 0; j < q.N; ++j) {
            const uint32_t b = q.blade[size_t(j)];
            const int k = __builtin_popcount(b);
            const bool held = ((l.mask >> k) & 1ULL) && int64_t(bt.index_of[b]) < l.grade_len(k);
            off.push_back(held ? int32_t(l.offset(k) + bt.index_of[b]) : -1);
        }
        return off;
    }
    // the sign words of ADJL and ADJR (Step::Inverse: adj_neg_l, adj_neg_r) from those of L
    static void adjoint_sign_words(Step::Inverse& q) {
        q.adj_neg_l.assign(size_t(q.N), 0);
        q.adj_neg_r.assign(size_t(q.N), 0);
        for (int j = 0; j < q.N; ++j)
            for (int t = 0; t < q.N; ++t)
                if ((q.neg[size_t(j ^ t)] >> t) & 1ULL) {   // the sign of L[j xor t][t]: coeff(a = j, b = t)
                    q.adj_neg_l[size_t(j)] |= uint64_t(1) << t;
                    q.adj_neg_r[size_t(t)] |= uint64_t(1) << j;
                }
    }

    // Reverse mode of the general exponential (GAAST_OP_GEXP_ADJ, gaast_hip.h): res += the cotangent of the operand, in the operand's
    // grades.  child1, the forward operand, is read like the forward's; child0, the cotangent, is cached like a product operand.
    // Reverse mode of the general square root (GAAST_OP_GSQRT_ADJ; Step::GSQRT_ADJ, k_mv_gsqrt_adj) has the same operands and the same
    // tables -- the two transposed sign words are the rows of the transposed L_X + R_X -- and is lowered by the same lines.  So is
    // reverse mode of the general logarithm (GAAST_OP_GLOG_ADJ; Step::GLOG_ADJ, k_mv_glog_adj), which uses the two words one at a time too.
    // GSQRT_ADJ alone produces its node's grades within the blade set, not only within the operand's grades (gaast_hip.h: the
    // second-order rule of gsqrt needs every component of the transposed solve); a node with the operand's mask lowers as it always did.
    void lower_gexp_adj(BufRef res, int id, Step::Kind kind, const std::string& op, const char* what, const char* label) {
        const gaast_node_desc& nd = node(id);
        const gaast_node_desc& ch = node(nd.child1);
        const int n = d.vec_space_dim;
        if (ch.vec_space_dim != n || nd.vec_space_dim != n || node(nd.child0).vec_space_dim != n) {
            fail(GAAST_ERR_INVALID_PROGRAM, op + " adjoint operand lives in another vector space than the algebra");
            return;
        }
        const uint64_t amask = ch.minimal_grade_mask & ((uint64_t(2) << n) - 1);
        const bool even = !(amask & 0xAAAAAAAAAAAAAAAAULL);
        if (blade_set_unsupported(what, even)) return;
        const uint64_t smask = gs_inverse(amask, n);
        if (node(nd.child0).minimal_grade_mask & ~smask) {
            fail(GAAST_ERR_INVALID_PROGRAM, op + " adjoint: the cotangent holds grades outside the blade set of the operand");
            return;
        }
        int canon = 0;
        uint64_t flip = 0;
        BufRef a = operand(nd.child1, &canon, &flip);
        if (!ok()) return;
        BufRef cot = store_in_cache(nd.child0);
        if (!ok()) return;
        if (key(a) == key(res) || key(cot) == key(res)) {
            fail(GAAST_ERR_MISSING_GRADE, op + " adjoint operand aliases its own result buffer");
            return;
        }
        const Layout &lg = layout(cot), &lr = layout(res);
        Step::Inverse q;
        if (!blade_set_tables(q, even, a, amask, flip, res, nd.minimal_grade_mask & (kind == Step::GSQRT_ADJ ? smask : amask))) return;
        q.wmax = 0.0;
        for (double w : q.weight) q.wmax = std::max(q.wmax, std::fabs(w));
        q.g_off = blade_offsets(q, lg);
        adjoint_sign_words(q);
        if (!q.n_out) return;
        const auto fr = fresh.find(key(res));
        const bool covers = fr != fresh.end() && !(plan.flags & GAAST_FLAG_NO_FUSION) && int64_t(q.n_out) == lr.row_len;
        if (covers) removed[size_t(fr->second)] = 1;
        Step& s = emit(kind, res, std::string(label) + "[" + std::to_string(q.N) + (even ? " even" : "") + " blades, " + std::to_string(q.n_out) + " produced, n=" + std::to_string(n) + "]");
        s.a = a;
        s.b = cot;
        s.canon_a = canon;
        s.beta = covers ? 0 : 1;
        s.inv = std::move(q);
        touch(res);
    }

    // The second-order steps of the general exponential (GAAST_OP_GEXP_JVP / GAAST_OP_GEXP_ADJ2, gaast_hip.h; Step::GEXP_JVP /
    // Step::GEXP_ADJ2, k_mv_gexp_jvp / k_mv_gexp_adj2), always launches of their own.  The forward operand (JVP: child1; ADJ2: the third
    // child, in input_slot) is read like GEXP_ADJ's; the tangent h (JVP: child0; ADJ2: child1) and ADJ2's g (child0) are cached like
    // product operands.  JVP: res += the wanted grades of the blade set; ADJ2: res += the operand's grades.
    void lower_gexp2(BufRef res, int id) {
        const gaast_node_desc& nd = node(id);
        const bool adj2 = nd.opcode == GAAST_OP_GEXP_ADJ2;
        const int a_id = adj2 ? nd.input_slot : nd.child1, h_id = adj2 ? nd.child1 : nd.child0, g_id = adj2 ? nd.child0 : -1;
        const std::string op = adj2 ? "gexp second-order adjoint" : "gexp tangent";
        const int n = d.vec_space_dim;
        if (node(a_id).vec_space_dim != n || nd.vec_space_dim != n || node(h_id).vec_space_dim != n || (adj2 && node(g_id).vec_space_dim != n)) {
            fail(GAAST_ERR_INVALID_PROGRAM, op + " operand lives in another vector space than the algebra");
            return;
        }
        const uint64_t amask = node(a_id).minimal_grade_mask & ((uint64_t(2) << n) - 1);
        const bool even = !(amask & 0xAAAAAAAAAAAAAAAAULL);
        if (blade_set_unsupported(adj2 ? "the general exponential's second-order adjoint" : "the general exponential's tangent", even)) return;
        const uint64_t smask = gs_inverse(amask, n);
        if (node(h_id).minimal_grade_mask & ~amask) {
            fail(GAAST_ERR_INVALID_PROGRAM, op + ": the tangent holds grades the operand does not hold");
            return;
        }
        if (adj2 ? (node(g_id).minimal_grade_mask & ~smask) != 0 : (nd.minimal_grade_mask & ~smask) != 0) {
            fail(GAAST_ERR_INVALID_PROGRAM, op + (adj2 ? ": the cotangent holds grades outside the blade set of the operand" : ": the node holds grades outside the blade set of the operand"));
            return;
        }
        int canon = 0;
        uint64_t flip = 0;
        BufRef a = operand(a_id, &canon, &flip);
        if (!ok()) return;
        BufRef h = store_in_cache(h_id);
        if (!ok()) return;
        BufRef g;
        if (adj2) g = store_in_cache(g_id);
        if (!ok()) return;
        if (key(a) == key(res) || key(h) == key(res) || (adj2 && key(g) == key(res))) {
            fail(GAAST_ERR_MISSING_GRADE, op + " operand aliases its own result buffer");
            return;
        }
        const Layout& lr = layout(res);
        Step::Inverse q;
        if (!blade_set_tables(q, even, a, amask, flip, res, adj2 ? nd.minimal_grade_mask & amask : nd.minimal_grade_mask)) return;
        q.wmax = 0.0;
        for (double w : q.weight) q.wmax = std::max(q.wmax, std::fabs(w));
        q.h_off = blade_offsets(q, layout(h));
        if (adj2) q.g_off = blade_offsets(q, layout(g));
        adjoint_sign_words(q);
        if (!q.n_out) return;
        const auto fr = fresh.find(key(res));
        const bool covers = fr != fresh.end() && !(plan.flags & GAAST_FLAG_NO_FUSION) && int64_t(q.n_out) == lr.row_len;
        if (covers) removed[size_t(fr->second)] = 1;
        Step& s = emit(adj2 ? Step::GEXP_ADJ2 : Step::GEXP_JVP, res, std::string(adj2 ? "general_exponential_adjoint2" : "general_exponential_jvp") + "[" + std::to_string(q.N) + (even ? " even" : "") + " blades, " + std::to_string(q.n_out) + " produced, n=" + std::to_string(n) + "]");
        s.a = a;
        s.b = g;
        s.c = h;
        s.canon_a = canon;
        s.beta = covers ? 0 : 1;
        s.inv = std::move(q);
        touch(res);
    }

    // The tangents of the general square root and logarithm (GAAST_OP_GSQRT_JVP / GAAST_OP_GLOG_JVP, gaast_hip.h; Step::GSQRT_JVP /
    // Step::GLOG_JVP, k_mv_gsqrt_jvp / k_mv_jvp_glog), always launches of their own.  child1, the forward operand, is read like the
    // adjoints'; child0, the tangent h (any grades of the blade set), is cached like a product operand.  res += the wanted grades of the
    // blade set.
    void lower_root_log_jvp(BufRef res, int id, Step::Kind kind, const std::string& op, const char* what, const char* label) {
        const gaast_node_desc& nd = node(id);
        const gaast_node_desc& ch = node(nd.child1);
        const int n = d.vec_space_dim;
        if (ch.vec_space_dim != n || nd.vec_space_dim != n || node(nd.child0).vec_space_dim != n) {
            fail(GAAST_ERR_INVALID_PROGRAM, op + " tangent operand lives in another vector space than the algebra");
            return;
        }
        const uint64_t amask = ch.minimal_grade_mask & ((uint64_t(2) << n) - 1);
        const bool even = !(amask & 0xAAAAAAAAAAAAAAAAULL);
        if (blade_set_unsupported(what, even)) return;
        const uint64_t smask = gs_inverse(amask, n);
        if (node(nd.child0).minimal_grade_mask & ~smask) {
            fail(GAAST_ERR_INVALID_PROGRAM, op + " tangent: the tangent holds grades outside the blade set of the operand");
            return;
        }
        int canon = 0;
        uint64_t flip = 0;
        BufRef a = operand(nd.child1, &canon, &flip);
        if (!ok()) return;
        BufRef h = store_in_cache(nd.child0);
        if (!ok()) return;
        if (key(a) == key(res) || key(h) == key(res)) {
            fail(GAAST_ERR_MISSING_GRADE, op + " tangent operand aliases its own result buffer");
            return;
        }
        const Layout& lr = layout(res);
        Step::Inverse q;
        if (!blade_set_tables(q, even, a, amask, flip, res, nd.minimal_grade_mask & smask)) return;
        q.wmax = 0.0;
        for (double w : q.weight) q.wmax = std::max(q.wmax, std::fabs(w));
        q.h_off = blade_offsets(q, layout(h));
        right_mul_sign_words(q);
        if (!q.n_out) return;
        const auto fr = fresh.find(key(res));
        const bool covers = fr != fresh.end() && !(plan.flags & GAAST_FLAG_NO_FUSION) && int64_t(q.n_out) == lr.row_len;
        if (covers) removed[size_t(fr->second)] = 1;
        Step& s = emit(kind, res, std::string(label) + "[" + std::to_string(q.N) + (even ? " even" : "") + " blades, " + std::to_string(q.n_out) + " produced, n=" + std::to_string(n) + "]");
        s.a = a;
        s.c = h;
        s.canon_a = canon;
        s.beta = covers ? 0 : 1;
        s.inv = std::move(q);
        touch(res);
    }
    // the sign words of the right-multiplication matrix (Step::Inverse: rmul_neg)
    static void right_mul_sign_words(Step::Inverse& q) {
        q.rmul_neg.assign(size_t(q.N), 0);
        for (int r = 0; r < q.N; ++r)
            for (int j = 0; j < q.N; ++j)
                if (reorder_parity(q.blade[size_t(j)], q.blade[size_t(r)] ^ q.blade[size_t(j)])) q.rmul_neg[size_t(r)] |= uint64_t(1) << j;
    }

    // The second-order adjoint of the general logarithm (GAAST_OP_GLOG_ADJ2, gaast_hip.h; Step::GLOG_ADJ2, k_mv_adj2_glog), always a launch
    // of its own.  The forward operand, the third child in input_slot, is read like the adjoint's; g (child0) and h (child1), any grades
    // of the blade set, are cached like product operands.  res += the operand's grades.  It needs all four sign tables.
    void lower_glog_adj2(BufRef res, int id) {
        const gaast_node_desc& nd = node(id);
        const int a_id = nd.input_slot, g_id = nd.child0, h_id = nd.child1;
        const std::string op = "glog second-order adjoint";
        const int n = d.vec_space_dim;
        if (node(a_id).vec_space_dim != n || nd.vec_space_dim != n || node(h_id).vec_space_dim != n || node(g_id).vec_space_dim != n) {
            fail(GAAST_ERR_INVALID_PROGRAM, op + " operand lives in another vector space than the algebra");
            return;
        }
        const uint64_t amask = node(a_id).minimal_grade_mask & ((uint64_t(2) << n) - 1);
        const bool even = !(amask & 0xAAAAAAAAAAAAAAAAULL);
        if (blade_set_unsupported("the general logarithm's second-order adjoint", even)) return;
        const uint64_t smask = gs_inverse(amask, n);
        if (node(h_id).minimal_grade_mask & ~smask) {
            fail(GAAST_ERR_INVALID_PROGRAM, op + ": the tangent holds grades outside the blade set of the operand");
            return;
        }
        if (node(g_id).minimal_grade_mask & ~smask) {
            fail(GAAST_ERR_INVALID_PROGRAM, op + ": the cotangent holds grades outside the blade set of the operand");
            return;
        }
        int canon = 0;
        uint64_t flip = 0;
        BufRef a = operand(a_id, &canon, &flip);
        if (!ok()) return;
        BufRef h = store_in_cache(h_id);
        if (!ok()) return;
        BufRef g = store_in_cache(g_id);
        if (!ok()) return;
        if (key(a) == key(res) || key(h) == key(res) || key(g) == key(res)) {
            fail(GAAST_ERR_MISSING_GRADE, op + " operand aliases its own result buffer");
            return;
        }
        const Layout& lr = layout(res);
        Step::Inverse q;
        if (!blade_set_tables(q, even, a, amask, flip, res, nd.minimal_grade_mask & amask)) return;
        q.wmax = 0.0;
        for (double w : q.weight) q.wmax = std::max(q.wmax, std::fabs(w));
        q.h_off = blade_offsets(q, layout(h));
        q.g_off = blade_offsets(q, layout(g));
        adjoint_sign_words(q);
        right_mul_sign_words(q);
        if (!q.n_out) return;
        const auto fr = fresh.find(key(res));
        const bool covers = fr != fresh.end() && !(plan.flags & GAAST_FLAG_NO_FUSION) && int64_t(q.n_out) == lr.row_len;
        if (covers) removed[size_t(fr->second)] = 1;
        Step& s = emit(Step::GLOG_ADJ2, res, std::string("general_log_adjoint2[") + std::to_string(q.N) + (even ? " even" : "") + " blades, " + std::to_string(q.n_out) + " produced, n=" + std::to_string(n) + "]");
        s.a = a;
        s.b = g;
        s.c = h;
        s.canon_a = canon;
        s.beta = covers ? 0 : 1;
        s.inv = std::move(q);
        touch(res);
    }

    // The general inverse (GAAST_OP_INV, gaast_hip.h; no reference counterpart): a one-operand product arm, always a launch of its
    // own (Step::INVERSE, k_mv_inverse).  The operand is read like a Product's (operand()); res += the Y with A Y = 1 in the wanted
    // grades.  Of a bare scalar it is ScalarInversion, arm for arm.
    void lower_inverse(BufRef res, int id) {
        const gaast_node_desc& nd = node(id);
        const gaast_node_desc& ch = node(nd.child0);
        const int n = d.vec_space_dim;
        if (ch.minimal_grade_mask == 1ULL) {   // eval.rs:103-110
            add_to_res(res, nd.child0);
            if (!ok()) return;
            const Layout& r = layout(res);
            if (!(r.mask & 1ULL)) {
                fail(GAAST_ERR_MISSING_GRADE, "scalar op on a buffer without grade 0");
                return;
            }
            Step& s = emit(Step::SUNARY, res, "scalar_inversion");
            s.sunary_op = 0;
            s.sunary_off = int(r.offset(0));
            touch(res);
            return;
        }
        if (ch.vec_space_dim != n || nd.vec_space_dim != n) {
            fail(GAAST_ERR_INVALID_PROGRAM, "inverse operand lives in another vector space than the algebra");
            return;
        }
        const uint64_t amask = ch.minimal_grade_mask & ((uint64_t(2) << n) - 1);
        const bool even = !(amask & 0xAAAAAAAAAAAAAAAAULL);
        if ((even ? n - 1 : n) > 6) {
            if (plan.unsupported.empty())
                plan.unsupported = "the general inverse over " + std::string(even ? "the even blades" : "every blade") + " of a " + std::to_string(n) +
                                   "-dimensional algebra: the elimination kernel is built for up to 64 blades";
            return;
        }
        int canon = 0;
        uint64_t flip = 0;
        BufRef a = operand(nd.child0, &canon, &flip);
        if (!ok()) return;
        if (key(a) == key(res)) {
            fail(GAAST_ERR_MISSING_GRADE, "inverse operand aliases its own result buffer");
            return;
        }
        const Layout& lr = layout(res);
        Step::Inverse q;
        if (!blade_set_tables(q, even, a, amask, flip, res, nd.minimal_grade_mask)) return;
        if (!q.n_out) return;
        // the first writer of a fresh buffer that covers every component of it: the zero fill is folded in
        const auto fr = fresh.find(key(res));
        const bool covers = fr != fresh.end() && !(plan.flags & GAAST_FLAG_NO_FUSION) && int64_t(q.n_out) == lr.row_len;
        if (covers) removed[size_t(fr->second)] = 1;
        Step& s = emit(Step::INVERSE, res, "inverse[" + std::to_string(q.N) + (even ? " even" : "") + " blades, " + std::to_string(q.n_out) + " produced, n=" + std::to_string(n) + "]");
        s.a = a;
        s.canon_a = canon;
        s.beta = covers ? 0 : 1;
        s.inv = std::move(q);
        plan.has_inverse = 1;
        touch(res);
    }

    // EXTENSION (GAAST_FLAG_EXP_LOG; eval.rs:112-113 is todo!() upstream, "no reference behaviour"): the semantics the
    // reference's grade rules imply (grade_set.rs:181-197), stated in oracle/gaast_oracle.c: ext_exp_log.  The operand is
    // cached like a product operand (eval.rs:67-68); res += exp / log of it.
    void lower_exp_log(BufRef res, int id) {
        const gaast_node_desc& nd = node(id);
        const bool is_exp = nd.opcode == GAAST_OP_EXP;
        const gaast_node_desc& ch = node(nd.child0);
        BufRef arg = store_in_cache(nd.child0);
        if (!ok()) return;
        if (key(arg) == key(res)) {
            fail(GAAST_ERR_MISSING_GRADE, "exp / log operand aliases its own result buffer");
            return;
        }
        int k = -1, nk = 0;
        for (int g = 0; g < 64; ++g) nk += int((ch.minimal_grade_mask >> g) & 1ULL);
        for (int g = 0; g < 64; ++g)
            if (((ch.minimal_grade_mask >> g) & 1ULL) && (g != 0 || (is_exp && nk == 1))) k = g;
        if (k < 0) {
            fail(GAAST_ERR_INVALID_PROGRAM, "log can only be used on multivectors of the form <A>_0 + <A>_k");
            return;
        }
        const Layout &la = layout(arg), &lr = layout(res);
        if (!((la.mask >> k) & 1ULL)) {
            fail(GAAST_ERR_MISSING_GRADE, "grade absent from exp / log operand");
            return;
        }
        const int dim = ch.vec_space_dim;
        if (dim != d.vec_space_dim) {
            fail(GAAST_ERR_INVALID_PROGRAM, "exp / log operand lives in another vector space than the algebra");
            return;
        }
        const int64_t m = la.grade_len(k);
        Step st;   // filled before emit(): emit invalidates references into plan.steps
        st.explog.op = is_exp ? 0 : 1;
        st.explog.m = int(m);
        st.explog.arg_k = int(la.offset(k));
        st.explog.arg_0 = (!is_exp && (la.mask & 1ULL) && la.grade_len(0) > 0) ? int(la.offset(0)) : -1;
        const uint64_t mine = nd.minimal_grade_mask;
        if (is_exp && (mine & 1ULL)) {
            if (!(lr.mask & 1ULL)) {
                fail(GAAST_ERR_MISSING_GRADE, "grade 0 absent from result buffer");
                return;
            }
            st.explog.res_0 = int(lr.offset(0));
        }
        // (exp of a bare scalar, k = 0: both statements land in grade 0, cosh|a| + (sinh|a| / |a|) a = e^a, as in the oracle)
        if ((mine >> k) & 1ULL) {
            if (!((lr.mask >> k) & 1ULL)) {
                fail(GAAST_ERR_MISSING_GRADE, "grade " + std::to_string(k) + " absent from result buffer");
                return;
            }
            st.explog.res_k = int(lr.offset(k));
            st.explog.mres = int(std::min<int64_t>(lr.grade_len(k), m));
        }
        // blade squares, and the pairs of commuting blades (the non-scalar part of B B) grouped by product blade
        std::vector<uint32_t> blade(static_cast<size_t>(m));
        for (int64_t i = 0; i < m; ++i) blade[size_t(i)] = bt.blade_of[size_t(k)][size_t(i)];
        st.explog.sq.resize(size_t(m));
        for (int64_t i = 0; i < m; ++i)
            st.explog.sq[size_t(i)] = blades_gp_coeff(d.vec_space_dim, d.metric_diag, blade[size_t(i)], blade[size_t(i)]);
        bool structurally_scalar = true;   // every pair of distinct grade-k blades anticommutes
        for (int64_t i = 0; i < m && structurally_scalar; ++i)
            for (int64_t j = i + 1; j < m; ++j)
                if (((k - __builtin_popcount(blade[size_t(i)] & blade[size_t(j)])) & 1) == 0) {
                    structurally_scalar = false;
                    break;
                }
        st.explog.row_start.assign(1, 0u);
        if (!structurally_scalar) {
            if (m > 512) {
                if (plan.unsupported.empty())
                    plan.unsupported = "exp / log of a " + std::to_string(m) + "-component k-vector: the domain check (square is scalar) is built for up to 512 components";
                return;
            }
            std::map<uint64_t, std::vector<std::pair<uint32_t, double>>> rows;   // T -> (i | j << 16, 2 e_i e_j), in (i, j) order
            for (int64_t i = 0; i < m; ++i)
                for (int64_t j = i + 1; j < m; ++j) {
                    const double c1 = blades_gp_coeff(d.vec_space_dim, d.metric_diag, blade[size_t(i)], blade[size_t(j)]);
                    const double c2 = blades_gp_coeff(d.vec_space_dim, d.metric_diag, blade[size_t(j)], blade[size_t(i)]);
                    if (c1 == c2) rows[uint64_t(blade[size_t(i)] ^ blade[size_t(j)])].push_back({uint32_t(i) | (uint32_t(j) << 16), 2.0 * c1});
                }
            for (auto& kv : rows) {
                for (auto& e : kv.second) {
                    st.explog.pairs.push_back(e.first);
                    st.explog.pair_coeff.push_back(e.second);
                }
                st.explog.row_start.push_back(uint32_t(st.explog.pairs.size()));
            }
        }
        Step& s = emit(Step::EXPLOG, res, std::string(is_exp ? "exponential" : "logarithm") + "[grade " + std::to_string(k) + ", " +
                                              std::to_string(m) + " components, " + std::to_string(st.explog.pairs.size()) + " domain-check pairs]");
        const BufRef keep_res = s.res;
        const std::string keep_name = s.name;
        s = std::move(st);
        s.kind = Step::EXPLOG;
        s.res = keep_res;
        s.name = keep_name;
        s.a = arg;
        plan.has_explog = 1;
        touch(res);
    }

    // Reverse mode of the extension (GAAST_OP_EXP_ADJ / GAAST_OP_LOG_ADJ, gaast_hip.h): res += the cotangent of the exp / log
    // operand.  Both children are cached like product operands -- child1 is the very operand buffer of the forward node when the
    // program re-evaluates it -- and the checks are lower_exp_log's.  No domain check: the forward made it.
    void lower_exp_log_adj(BufRef res, int id) {
        const gaast_node_desc& nd = node(id);
        const bool is_exp = nd.opcode == GAAST_OP_EXP_ADJ;
        if (!(plan.flags & GAAST_FLAG_EXP_LOG)) {   // refused whole at program_create, like every program beyond this back end
            if (plan.unsupported.empty()) plan.unsupported = "exp / log adjoint nodes need GAAST_FLAG_EXP_LOG";
            return;
        }
        const gaast_node_desc& ch = node(nd.child1);
        BufRef arg = store_in_cache(nd.child1);
        if (!ok()) return;
        BufRef cot = store_in_cache(nd.child0);
        if (!ok()) return;
        if (key(arg) == key(res) || key(cot) == key(res)) {
            fail(GAAST_ERR_MISSING_GRADE, "exp / log adjoint operand aliases its own result buffer");
            return;
        }
        int k = -1, nk = 0;
        for (int g = 0; g < 64; ++g) nk += int((ch.minimal_grade_mask >> g) & 1ULL);
        for (int g = 0; g < 64; ++g)
            if (((ch.minimal_grade_mask >> g) & 1ULL) && (g != 0 || (is_exp && nk == 1))) k = g;
        if (k < 0) {
            fail(GAAST_ERR_INVALID_PROGRAM, "log can only be used on multivectors of the form <A>_0 + <A>_k");
            return;
        }
        if (k == 0) {
            if (plan.unsupported.empty()) plan.unsupported = "exp of a bare scalar has no adjoint node";
            return;
        }
        const Layout &la = layout(arg), &lg = layout(cot), &lr = layout(res);
        if (!((la.mask >> k) & 1ULL)) {
            fail(GAAST_ERR_MISSING_GRADE, "grade absent from exp / log operand");
            return;
        }
        if (ch.vec_space_dim != d.vec_space_dim || lg.dim != d.vec_space_dim) {
            fail(GAAST_ERR_INVALID_PROGRAM, "exp / log adjoint operand lives in another vector space than the algebra");
            return;
        }
        const int64_t m = la.grade_len(k);
        Step st;   // filled before emit(): emit invalidates references into plan.steps
        st.adj.op = is_exp ? 0 : 1;
        st.adj.m = int(m);
        st.adj.arg_k = int(la.offset(k));
        st.adj.arg_0 = (!is_exp && (la.mask & 1ULL) && la.grade_len(0) > 0) ? int(la.offset(0)) : -1;
        if ((lg.mask >> k) & 1ULL) {
            st.adj.g_k = int(lg.offset(k));
            st.adj.mg = int(std::min<int64_t>(lg.grade_len(k), m));
        }
        if (is_exp && (lg.mask & 1ULL) && lg.grade_len(0) > 0) st.adj.g_0 = int(lg.offset(0));
        const uint64_t mine = nd.minimal_grade_mask;
        if ((mine >> k) & 1ULL) {
            if (!((lr.mask >> k) & 1ULL)) {
                fail(GAAST_ERR_MISSING_GRADE, "grade " + std::to_string(k) + " absent from result buffer");
                return;
            }
            st.adj.res_k = int(lr.offset(k));
            st.adj.mres = int(std::min<int64_t>(lr.grade_len(k), m));
        }
        if (st.adj.arg_0 >= 0 && (mine & 1ULL)) {
            if (!(lr.mask & 1ULL)) {
                fail(GAAST_ERR_MISSING_GRADE, "grade 0 absent from result buffer");
                return;
            }
            st.adj.res_0 = int(lr.offset(0));
        }
        st.adj.sq.resize(size_t(m));
        for (int64_t i = 0; i < m; ++i) {
            const uint32_t blade = bt.blade_of[size_t(k)][size_t(i)];
            st.adj.sq[size_t(i)] = blades_gp_coeff(d.vec_space_dim, d.metric_diag, blade, blade);
        }
        Step& s = emit(Step::EXPLOG_ADJ, res, std::string(is_exp ? "exponential_adjoint" : "logarithm_adjoint") + "[grade " + std::to_string(k) + ", " +
                                                  std::to_string(m) + " components]");
        const BufRef keep_res = s.res;
        const std::string keep_name = s.name;
        s = std::move(st);
        s.kind = Step::EXPLOG_ADJ;
        s.res = keep_res;
        s.name = keep_name;
        s.a = arg;
        s.b = cot;
        plan.has_explog_adj = 1;
        touch(res);
    }

    // Which buffer a Product reads for operand `id`.  Exact rewrites (off with NO_FUSION):
    //  - a bound input holding every wanted grade is read in place (canon: 0.0 + x);
    //  - a chain of sign-only arms (Negation / Reverse / GradeInvolution / GradeProjection) over
    //    such an input is not materialised either: the grades it negates are returned in *flip
    //    and folded into the comp-mul coefficients -- ((-l) * r) * c == (l * r) * (-c) bit for bit.
    BufRef operand(int id, int* canon, uint64_t* flip) {
        *canon = 0;
        *flip = 0;
        if (!(plan.flags & GAAST_FLAG_NO_FUSION) && cache[size_t(id)] < 0) {
            uint64_t f = 0;
            int cur = id;
            bool ok_chain = true;
            while (node(cur).opcode != GAAST_OP_INPUT) {
                const gaast_node_desc& nd = node(cur);
                const uint64_t gs = nd.minimal_grade_mask;
                const bool sign_only = nd.opcode == GAAST_OP_NEG || nd.opcode == GAAST_OP_REVERSE ||
                                       nd.opcode == GAAST_OP_GINVOL || nd.opcode == GAAST_OP_PROJ;
                // the child must fill exactly the grades this node's buffer would have (Q2 otherwise)
                if (!sign_only || node(nd.child0).minimal_grade_mask != gs || gs == 0) {
                    ok_chain = false;
                    break;
                }
                if (nd.opcode == GAAST_OP_REVERSE && (gs & 1ULL) && (plan.flags & GAAST_FLAG_DEBUG_OVERFLOW)) {
                    ok_chain = false;  // let the materialising path report the panic
                    break;
                }
                for (int k = 0; k < 64; ++k) {
                    if (!((gs >> k) & 1ULL)) continue;
                    const bool neg = nd.opcode == GAAST_OP_NEG || (nd.opcode == GAAST_OP_REVERSE && (k % 4 == 2 || k % 4 == 3)) ||
                                     (nd.opcode == GAAST_OP_GINVOL && (k & 1));
                    if (neg) f ^= 1ULL << k;
                }
                cur = nd.child0;
            }
            if (ok_chain && direct_input_ok(cur)) {
                *canon = 1;
                *flip = f;
                return BufRef{BufKind::INPUT, node(cur).input_slot};
            }
        }
        return store_in_cache(id);  // eval.rs:67-68
    }

    // What the three paths of a Product share; then the opt-in matrix-representation kernels, a dense kernel (both plan_dense.cpp),
    // or the exact list
    void lower_product(BufRef res, int id) {  // eval.rs:61-86
        const gaast_node_desc& nd = node(id);
        int canon_l = 0, canon_r = 0;
        uint64_t flip_l = 0, flip_r = 0;
        BufRef l = operand(nd.child0, &canon_l, &flip_l);
        if (!ok()) return;
        BufRef r = operand(nd.child1, &canon_r, &flip_r);
        if (!ok()) return;
        if (key(l) == key(res) || key(r) == key(res)) {
            fail(GAAST_ERR_MISSING_GRADE, "product operand aliases its own result buffer");
            return;
        }
        if (nd.comp_muls == nullptr && nd.product_kind < 0)
            throw std::runtime_error("PRODUCT node has neither a comp-mul list nor a product kind");
        // may the zero-fill of a fresh result buffer be folded into this product?
        const auto fr = fresh.find(key(res));
        const bool is_fresh = fr != fresh.end() && !(plan.flags & GAAST_FLAG_NO_FUSION);
        const ProductOperands po{nd, res, l, r, canon_l, canon_r, flip_l, flip_r, node(nd.child0).minimal_grade_mask, node(nd.child1).minimal_grade_mask,
                                 is_fresh ? fr->second : -1};
        DenseChoice choice;
        const bool spinor = spinor_eligible(*this, po);
        if (spinor || dense_choice(*this, po, choice)) {
            if ((nd.minimal_grade_mask & layout(res).mask) != nd.minimal_grade_mask) {
                fail(GAAST_ERR_MISSING_GRADE, "product result grade absent from result buffer");
                return;
            }
            if (spinor) lower_product_spinor(*this, po);
            else lower_product_dense(*this, po, choice);
            return;
        }
        lower_product_list(po);
    }

    // ---- exact path: CSR by output component, entries in the reference's order ----
    void lower_product_list(const ProductOperands& po) {
        const gaast_node_desc& nd = po.nd;
        const BufRef res = po.res, l = po.l, r = po.r;
        const Layout &lr = layout(res), &ll = layout(l), &lrr = layout(r);
        const uint64_t lmin = po.lmin, rmin = po.rmin, omin = nd.minimal_grade_mask;
        const uint64_t flip_l = po.flip_l, flip_r = po.flip_r;
        // (a regressive list -- generated here, or explicit and naming its kind -- takes the orientation sign of a Gram basis)
        const bool regressive = nd.product_kind >= 0 && (nd.product_kind & 7) == GAAST_PROD_REGRESSIVE;
        const bool mirror_list = regressive && plan.mirrored;
        std::vector<gaast_comp_mul> generated;
        const gaast_comp_mul* muls = nd.comp_muls;
        uint64_t n_muls = nd.n_comp_muls;
        {
            // capability limits, checked BEFORE any table is generated: the list kernels stage both operand rows of
            // an item in LDS, and the list itself has to fit the table budget
            const size_t elem = plan.dtype == GAAST_F32 ? 4 : 8;
            const size_t per_item = size_t(ll.row_len + lrr.row_len) * elem;
            const bool fits_fused_slab = ll.row_len + lrr.row_len + lr.row_len < 4096;
            if (per_item > kLdsBytes && !fits_fused_slab && plan.unsupported.empty())
                plan.unsupported = "product operands of " + std::to_string(per_item) + " bytes per item exceed the " +
                                   std::to_string(kLdsBytes) + "-byte LDS the list kernels stage them in";
            if (n_muls > kMaxListEntries && plan.unsupported.empty())
                plan.unsupported = "a comp-mul list of " + std::to_string(n_muls) + " entries exceeds this back end's table budget";
            if (!plan.unsupported.empty()) return;
        }
        if (!muls && nd.product_kind >= GAAST_PROD_ADJ_LEFT) {
            // compact adjoint: regenerate the forward list from the node's three grade sets, then transpose it
            const bool right = (nd.product_kind & GAAST_PROD_ADJ_RIGHT) != 0;
            const Selection sel{nd.product_kind & 7, nullptr, nullptr, d.vec_space_dim};
            auto contribs = right ? iter_contribs(lmin, sel, rmin, omin) : iter_contribs(lmin, sel, omin, rmin);
            const uint64_t count = comp_mul_count(d.vec_space_dim, contribs, regressive);
            // no dense kernel took it (EXACT_ORDER, a kind other than geometric, a metric the kernels cannot scale): the list is
            // regenerated, transposed and sorted on the host -- refused beyond kMaxAdjointListEntries instead of building GBs
            if (count > kMaxAdjointListEntries && plan.unsupported.empty())
                plan.unsupported = "a compact adjoint product whose list of " + std::to_string(count) +
                                   " entries no dense kernel takes exceeds the adjoint list budget";
            if (!plan.unsupported.empty()) return;
            std::vector<gaast_comp_mul> fwd;
            fwd.reserve(size_t(count));
            for_each_comp_mul(bt, d.metric_diag, contribs, [&](const gaast_comp_mul& m) { fwd.push_back(m); }, regressive);
            generated = transpose_comp_muls(fwd.data(), fwd.size(), right, true);
            muls = generated.data();
            n_muls = generated.size();
        }
        if (!muls) {
            Selection sel{nd.product_kind, nullptr, nullptr, d.vec_space_dim};
            auto contribs = iter_contribs(omin, sel, lmin, rmin);
            if (comp_mul_count(d.vec_space_dim, contribs, regressive) > kMaxListEntries && plan.unsupported.empty())
                plan.unsupported = "a comp-mul list of " + std::to_string(comp_mul_count(d.vec_space_dim, contribs, regressive)) +
                                   " entries exceeds this back end's table budget";
            if (!plan.unsupported.empty()) return;
            generated.reserve(size_t(comp_mul_count(d.vec_space_dim, contribs, regressive)));
            for_each_comp_mul(bt, d.metric_diag, contribs,
                              [&](const gaast_comp_mul& m) { generated.push_back(m); }, regressive);
            muls = generated.data();
            n_muls = generated.size();
        }
        if (n_muls == 0) return;  // nothing is added to res
        if (ll.row_len > 65536 || lrr.row_len > 65536) throw std::runtime_error("operand row too long");

        const bool beta0 = po.fresh_zero >= 0;
        // rows: with beta0 every component of the result row gets a row (empty rows write 0.0)
        std::vector<int32_t> row_of(size_t(lr.row_len), -1);
        std::vector<uint32_t> row_out, counts;
        if (beta0)
            for (int64_t o = 0; o < lr.row_len; ++o) {
                row_of[size_t(o)] = int32_t(row_out.size());
                row_out.push_back(uint32_t(o));
                counts.push_back(0);
            }
        std::vector<uint32_t> eo(static_cast<size_t>(n_muls), 0u);  // output offset of each entry
        for (uint64_t e = 0; e < n_muls; ++e) {
            const gaast_comp_mul& m = muls[e];
            auto check = [&](const Layout& lay, uint32_t g, uint32_t i, const char* what) -> int64_t {
                if (g >= 64 || !((lay.mask >> g) & 1ULL)) {
                    fail(GAAST_ERR_MISSING_GRADE, std::string("grade absent from product ") + what);
                    return -1;
                }
                if (int64_t(i) >= lay.grade_len(int(g))) throw std::runtime_error("comp-mul index out of range");
                return lay.offset(int(g)) + i;
            };
            const int64_t lo = check(ll, m.left_grade, m.left_index, "left operand");
            const int64_t ro = check(lrr, m.right_grade, m.right_index, "right operand");
            const int64_t oo = check(lr, m.result_grade, m.result_index, "result");
            if (lo < 0 || ro < 0 || oo < 0) return;
            if (row_of[size_t(oo)] < 0) {
                row_of[size_t(oo)] = int32_t(row_out.size());
                row_out.push_back(uint32_t(oo));
                counts.push_back(0);
            }
            counts[size_t(row_of[size_t(oo)])]++;
            eo[size_t(e)] = uint32_t(oo);
        }
        if (beta0) removed[size_t(po.fresh_zero)] = 1;
        Step& s = emit(Step::PRODUCT_CSR, res, "product_csr[" + std::to_string(n_muls) + " comp-muls]");
        s.a = l;
        s.b = r;
        s.canon_a = po.canon_l;
        s.canon_b = po.canon_r;
        s.beta = beta0 ? 0 : 1;
        s.n_entries = n_muls;
        s.list.row_start.assign(row_out.size() + 1, 0);
        for (size_t i = 0; i < counts.size(); ++i) s.list.row_start[i + 1] = s.list.row_start[i] + counts[i];
        s.list.row_out = row_out;
        s.list.entries.resize(size_t(n_muls));
        s.list.coeff.resize(size_t(n_muls));
        std::vector<uint32_t> cursor(s.list.row_start.begin(), s.list.row_start.end() - 1);
        for (uint64_t e = 0; e < n_muls; ++e) {  // stable: keeps the reference order per output
            const gaast_comp_mul& m = muls[e];
            const uint32_t pos = cursor[size_t(row_of[eo[size_t(e)]])]++;
            const uint32_t lo = uint32_t(ll.offset(int(m.left_grade)) + m.left_index);
            const uint32_t ro = uint32_t(lrr.offset(int(m.right_grade)) + m.right_index);
            s.list.entries[pos] = lo | (ro << 16);
            const bool neg = ((((flip_l >> m.left_grade) ^ (flip_r >> m.right_grade)) & 1ULL) != 0) != mirror_list;
            s.list.coeff[pos] = neg ? -m.coeff : m.coeff;
        }
        touch(res);
    }
};

}  // namespace

void build_plan(const gaast_program_desc& desc, Plan& plan, bool small_reg_slab, bool mirrored) {
    plan.mirrored = mirrored ? 1 : 0;
    if (desc.vec_space_dim < 0 || desc.vec_space_dim > GAAST_MAX_DIM) throw std::runtime_error("vec_space_dim out of range");
    if (desc.n_nodes <= 0 || desc.root < 0 || desc.root >= desc.n_nodes) throw std::runtime_error("bad node count / root");
    if (desc.dtype != GAAST_F64 && desc.dtype != GAAST_F32) throw std::runtime_error("bad dtype");
    if (desc.n_inputs < 0 || desc.n_inputs > GAAST_MAX_INPUTS) throw std::runtime_error("too many inputs");
    plan.n = desc.vec_space_dim;
    plan.dtype = desc.dtype;
    plan.flags = desc.flags;
    plan.metric.assign(desc.metric_diag, desc.metric_diag + desc.vec_space_dim);
    plan.inputs.assign(desc.inputs, desc.inputs + desc.n_inputs);
    plan.const_rows.resize(size_t(desc.n_inputs));
    plan.input_layouts.resize(size_t(desc.n_inputs));
    for (int i = 0; i < desc.n_inputs; ++i) {
        const gaast_input_desc& in = desc.inputs[i];
        if (in.storage_dim < 0 || in.storage_dim > GAAST_MAX_DIM) throw std::runtime_error("input storage_dim out of range");
        plan.input_layouts[size_t(i)] = make_layout(in.storage_dim, in.grade_mask);
        if (in.is_const) {
            const int64_t len = plan.input_layouts[size_t(i)].row_len;
            if (len && !in.const_row) throw std::runtime_error("constant input without data");
            plan.const_rows[size_t(i)].assign(in.const_row, in.const_row + len);
            plan.inputs[size_t(i)].const_row = nullptr;  // no host pointer is retained
        }
    }
    for (int i = 0; i < desc.n_nodes; ++i) {
        const gaast_node_desc& nd = desc.nodes[i];
        auto child_ok = [&](int c) { return c >= 0 && c < i; };
        switch (nd.opcode) {
        case GAAST_OP_INPUT:
            if (nd.input_slot < 0 || nd.input_slot >= desc.n_inputs) throw std::runtime_error("input slot out of range");
            break;
        case GAAST_OP_ADD:
        case GAAST_OP_PRODUCT:
        case GAAST_OP_EXP_ADJ:
        case GAAST_OP_LOG_ADJ:
        case GAAST_OP_GEXP_ADJ:
        case GAAST_OP_GSQRT_ADJ:
        case GAAST_OP_GLOG_ADJ:
        case GAAST_OP_GEXP_JVP:
        case GAAST_OP_GEXP_ADJ2:
        case GAAST_OP_GSQRT_JVP:
        case GAAST_OP_GLOG_JVP:
        case GAAST_OP_GLOG_ADJ2:
            if (!child_ok(nd.child0) || !child_ok(nd.child1)) throw std::runtime_error("nodes are not in post-order");
            if ((nd.opcode == GAAST_OP_GEXP_ADJ2 || nd.opcode == GAAST_OP_GLOG_ADJ2) && !child_ok(nd.input_slot)) throw std::runtime_error("nodes are not in post-order");   // (its third child)
            if (nd.opcode == GAAST_OP_PRODUCT && nd.product_kind >= GAAST_PROD_ADJ_LEFT) {
                const int adj = nd.product_kind & ~7, base = nd.product_kind & 7;
                if ((adj != GAAST_PROD_ADJ_LEFT && adj != GAAST_PROD_ADJ_RIGHT) || base > GAAST_PROD_REGRESSIVE)
                    throw std::runtime_error("unknown product kind");
            }
            break;
        case GAAST_OP_NEG: case GAAST_OP_EXP: case GAAST_OP_LOG: case GAAST_OP_PROJ:
        case GAAST_OP_REVERSE: case GAAST_OP_GINVOL: case GAAST_OP_SINV: case GAAST_OP_SSQRT:
        case GAAST_OP_DUAL: case GAAST_OP_UNDUAL: case GAAST_OP_INV: case GAAST_OP_GEXP: case GAAST_OP_GSQRT: case GAAST_OP_GLOG:
            if (!child_ok(nd.child0)) throw std::runtime_error("nodes are not in post-order");
            break;
        default: throw std::runtime_error("unknown opcode");
        }
        if (nd.vec_space_dim < 0 || nd.vec_space_dim > GAAST_MAX_DIM) throw std::runtime_error("node dim out of range");
    }

    Lowering lw(desc, plan);
    // eval.rs:12-19: the root is cached like any other node; its buffer is the caller's `out`
    const gaast_node_desc& root = desc.nodes[desc.root];
    plan.out_layout = make_layout(root.vec_space_dim, root.minimal_grade_mask);
    BufRef out{BufKind::OUT, 0};
    lw.emit_zero(out);
    lw.add_to_res(out, desc.root);
    // drop the zero-fills that were folded into products
    std::vector<Step> kept;
    for (size_t i = 0; i < plan.steps.size(); ++i)
        if (!lw.removed[i]) kept.push_back(std::move(plan.steps[i]));
    plan.steps = std::move(kept);
    plan.node_dead.assign(plan.node_buffers.size(), 0);
    // A program that would only fit the LDS interpreter (its slab is beyond the registers of the hiprtc-specialised kernel) but is
    // exactly one list chain -- (R X ~R).g(1) at n = 8 -- runs on k_product_ell_chain instead (same box: 1.43 against 1.59 ms per 1 M items)
    const int slab = fused_slab(plan, small_reg_slab);
    if (slab > (plan.dtype == GAAST_F32 ? 200 : 160) && !(plan.flags & (GAAST_FLAG_NO_FUSION | GAAST_FLAG_DEBUG_NO_CHAIN | GAAST_FLAG_NO_JIT))) {
        Plan trial = plan;
        uniform_csr_to_ell(trial);
        chain_list_into_list(trial);
        if (trial.steps.size() == 1 && trial.steps[0].chain.side) {
            plan = std::move(trial);
            return;
        }
    }
    if (!try_fuse(plan, small_reg_slab)) run_plan_passes(plan);
}

}  // namespace gaast
