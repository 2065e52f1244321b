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
        case GAAST_OP_GEXP: lower_gexp(res, id); return;
        case GAAST_OP_GEXP_ADJ: lower_gexp_adj(res, id); return;
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

    // The tables of a step over the blade set S (Step::Inverse: INVERSE, GEXP, GEXP_ADJ): S itself, where operand row `a` (grades
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

    // is a general exponential over this blade set beyond the kernels (N = 2 ... 64)?  Then the plan is marked unsupported
    bool blade_set_unsupported(const char* what, bool even) {
        const int n = d.vec_space_dim, bits = even ? n - 1 : n;
        if (bits >= 1 && bits <= 6) return false;
        if (plan.unsupported.empty())
            plan.unsupported = std::string(what) + " over " + (even ? "the even blades" : "every blade") + " of a " + std::to_string(n) +
                               "-dimensional algebra: the kernel is built for 2 to 64 blades";
        return true;
    }

    // The general exponential (GAAST_OP_GEXP, gaast_hip.h; no reference counterpart): a one-operand product arm, always a launch of
    // its own (Step::GEXP, k_mv_gexp).  The operand is read like the inverse's; res += exp(A) in the wanted grades.
    void lower_gexp(BufRef res, int id) {
        const gaast_node_desc& nd = node(id);
        const gaast_node_desc& ch = node(nd.child0);
        const int n = d.vec_space_dim;
        if (ch.vec_space_dim != n || nd.vec_space_dim != n) {
            fail(GAAST_ERR_INVALID_PROGRAM, "gexp operand lives in another vector space than the algebra");
            return;
        }
        const uint64_t amask = ch.minimal_grade_mask & ((uint64_t(2) << n) - 1);
        const bool even = !(amask & 0xAAAAAAAAAAAAAAAAULL);
        if (blade_set_unsupported("the general exponential", even)) return;
        int canon = 0;
        uint64_t flip = 0;
        BufRef a = operand(nd.child0, &canon, &flip);
        if (!ok()) return;
        if (key(a) == key(res)) {
            fail(GAAST_ERR_MISSING_GRADE, "gexp operand aliases its own result buffer");
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
        Step& s = emit(Step::GEXP, res, "general_exponential[" + std::to_string(q.N) + (even ? " even" : "") + " blades, " + std::to_string(q.n_out) + " produced, n=" + std::to_string(n) + "]");
        s.a = a;
        s.canon_a = canon;
        s.beta = covers ? 0 : 1;
        s.inv = std::move(q);
        plan.has_gexp = 1;
        touch(res);
    }

    // Reverse mode of the general exponential (GAAST_OP_GEXP_ADJ, gaast_hip.h): res += the cotangent of the operand, in the operand's
    // grades.  child1, the forward operand, is read like the forward's; child0, the cotangent, is cached like a product operand.
    void lower_gexp_adj(BufRef res, int id) {
        const gaast_node_desc& nd = node(id);
        const gaast_node_desc& ch = node(nd.child1);
        const int n = d.vec_space_dim;
        if (ch.vec_space_dim != n || nd.vec_space_dim != n || node(nd.child0).vec_space_dim != n) {
            fail(GAAST_ERR_INVALID_PROGRAM, "gexp adjoint operand lives in another vector space than the algebra");
            return;
        }
        const uint64_t amask = ch.minimal_grade_mask & ((uint64_t(2) << n) - 1);
        const bool even = !(amask & 0xAAAAAAAAAAAAAAAAULL);
        if (blade_set_unsupported("the general exponential's adjoint", even)) return;
        const uint64_t smask = gs_inverse(amask, n);
        if (node(nd.child0).minimal_grade_mask & ~smask) {
            fail(GAAST_ERR_INVALID_PROGRAM, "gexp adjoint: the cotangent holds grades outside the blade set of the operand");
            return;
        }
        int canon = 0;
        uint64_t flip = 0;
        BufRef a = operand(nd.child1, &canon, &flip);
        if (!ok()) return;
        BufRef cot = store_in_cache(nd.child0);
        if (!ok()) return;
        if (key(a) == key(res) || key(cot) == key(res)) {
            fail(GAAST_ERR_MISSING_GRADE, "gexp adjoint operand aliases its own result buffer");
            return;
        }
        const Layout &lg = layout(cot), &lr = layout(res);
        Step::Inverse q;
        if (!blade_set_tables(q, even, a, amask, flip, res, nd.minimal_grade_mask & amask)) return;
        q.wmax = 0.0;
        for (double w : q.weight) q.wmax = std::max(q.wmax, std::fabs(w));
        q.adj_neg_l.assign(size_t(q.N), 0);
        q.adj_neg_r.assign(size_t(q.N), 0);
        for (int j = 0; j < q.N; ++j) {
            const uint32_t b = q.blade[size_t(j)];
            const int k = __builtin_popcount(b);
            const bool held = ((lg.mask >> k) & 1ULL) && int64_t(bt.index_of[b]) < lg.grade_len(k);
            q.g_off.push_back(held ? int32_t(lg.offset(k) + bt.index_of[b]) : -1);
            for (int t = 0; t < q.N; ++t)
                if ((q.neg[size_t(j ^ t)] >> t) & 1ULL) {   // the sign of L[j xor t][t]: coeff(a = j, b = t)
                    q.adj_neg_l[size_t(j)] |= uint64_t(1) << t;
                    q.adj_neg_r[size_t(t)] |= uint64_t(1) << j;
                }
        }
        if (!q.n_out) return;
        const auto fr = fresh.find(key(res));
        const bool covers = fr != fresh.end() && !(plan.flags & GAAST_FLAG_NO_FUSION) && int64_t(q.n_out) == lr.row_len;
        if (covers) removed[size_t(fr->second)] = 1;
        Step& s = emit(Step::GEXP_ADJ, res, "general_exponential_adjoint[" + std::to_string(q.N) + (even ? " even" : "") + " blades, " + std::to_string(q.n_out) + " produced, n=" + std::to_string(n) + "]");
        s.a = a;
        s.b = cot;
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

// Rows of one length with +-1 coefficients (dense products of non-degenerate algebras) that were not fused
// into a small-program launch: the same lists transposed to [term][row] with the sign in bit 31 --
// consecutive threads (rows) then read consecutive words and no coefficient array is streamed
// (k_product_ell).  Same order, same roundings: (l * r) * (-1.0) is -(l * r) exactly.
static void uniform_csr_to_ell(Plan& plan) {
    if (plan.flags & GAAST_FLAG_NO_FUSION) return;
    for (Step& s : plan.steps) {
        if (s.kind != Step::PRODUCT_CSR || s.list.row_out.empty()) continue;
        const size_t n_rows = s.list.row_out.size();
        const uint32_t width = s.list.row_start[1] - s.list.row_start[0];
        bool uniform = width >= 4;   // (round 3: from 4 terms per row on -- R X has n per row; 16 before: such lists ran on k_product_csr, an entry and a coefficient load per term)
        for (size_t i = 0; uniform && i < n_rows; ++i) uniform = s.list.row_start[i + 1] - s.list.row_start[i] == width;
        for (size_t e = 0; uniform && e < s.list.coeff.size(); ++e) uniform = s.list.coeff[e] == 1.0 || s.list.coeff[e] == -1.0;
        for (size_t e = 0; uniform && e < s.list.entries.size(); ++e) uniform = !(s.list.entries[e] & 0x80000000u);   // right offset < 2^15
        if (!uniform) continue;
        // offsets in BYTES when they fit 15 bits (rows of <= 32 KiB: n <= 12 in f64, n <= 13 in f32): the kernel
        // then adds them to an LDS base without scaling
        const uint32_t elem = plan.dtype == GAAST_F32 ? 4u : 8u;
        bool bytes = true;
        for (size_t e = 0; bytes && e < s.list.entries.size(); ++e)
            bytes = (s.list.entries[e] & 0xffffu) * elem < 32768u && (s.list.entries[e] >> 16) * elem < 32768u;
        std::vector<uint32_t> ell(size_t(width) * n_rows);
        for (size_t row = 0; row < n_rows; ++row)
            for (uint32_t t = 0; t < width; ++t) {
                const size_t e = size_t(s.list.row_start[row]) + t;
                const uint32_t lo = s.list.entries[e] & 0xffffu, ro = s.list.entries[e] >> 16;
                const uint32_t word = bytes ? (lo * elem) | ((ro * elem) << 16) : s.list.entries[e];
                ell[size_t(t) * n_rows + row] = word | (s.list.coeff[e] < 0.0 ? 0x80000000u : 0u);
            }
        s.list.ell_bytes = bytes ? 1 : 0;
        s.list.entries.swap(ell);
        s.list.coeff.clear();
        s.list.ell_width = int(width);
        s.name = "product_ell" + s.name.substr(s.name.find('['));
    }
}

// A sparse product whose result is read ONLY as the left operand of a dense product (R X in R X ~R, eval.rs:61-86 with its
// cached operand) is evaluated inside the dense kernel, in LDS, while that kernel stages its operands: one launch instead of
// two, and the intermediate row never goes through HBM (BASELINE configs[4] at the dimensions where the whole program no
// longer fits a fused small-program kernel).  The list keeps the reference's order and roundings, so the dense kernel sees
// the very bits the separate launch would have written.  Off with GAAST_FLAG_DEBUG_NO_CHAIN (A/B, tests).
static void chain_sparse_into_dense(Plan& plan) {
    if (plan.flags & (GAAST_FLAG_NO_FUSION | GAAST_FLAG_DEBUG_NO_CHAIN)) return;
    plan.node_dead.assign(plan.node_buffers.size(), 0);
    const size_t elem = plan.dtype == GAAST_F32 ? 4 : 8;
    for (size_t j = 0; j < plan.steps.size(); ++j) {
        Step& dn = plan.steps[j];
        const DenseFamily fam = dn.dense.family;   // (k_gp_mfma6 has no chained staging: programs that small are fused whole)
        if (dn.kind != Step::PRODUCT_DENSE || fam == DenseFamily::SPINOR || fam == DenseFamily::MFMA6 || dn.dense.chained || dn.a.kind != BufKind::NODE) continue;
        const BufRef buf = dn.a;
        // exactly one writer (a list product that starts the buffer: beta = 0), no other reader, nothing else touches it
        int writer = -1;
        bool ok = dn.b != buf;
        for (size_t i = 0; i < plan.steps.size() && ok; ++i) {
            const Step& t = plan.steps[i];
            if (i == j) continue;
            if (t.kind == Step::FUSED) ok = false;
            if (t.res == buf) {
                if (writer >= 0 || t.kind != Step::PRODUCT_CSR || t.beta != 0 || i > j) ok = false;
                writer = int(i);
            }
            if (reads(t, buf)) ok = false;
        }
        if (!ok || writer < 0) continue;
        Step& w = plan.steps[size_t(writer)];
        // the list's operands must still hold at the dense launch: inputs always do; a cache buffer does unless a later step
        // writes it (cache buffers are written by the steps that fill them, all before their first reader)
        for (size_t i = size_t(writer) + 1; i < j && ok; ++i)
            if (plan.steps[i].res == w.a || plan.steps[i].res == w.b) ok = false;
        if (!ok) continue;
        auto row_len = [&](BufRef r) -> int64_t {
            return r.kind == BufKind::NODE ? plan.node_buffers[size_t(r.idx)].row_len : r.kind == BufKind::INPUT ? plan.input_layouts[size_t(r.idx)].row_len
                                                                                                               : plan.out_layout.row_len;
        };
        const int64_t ll = row_len(w.a), rl = row_len(w.b);
        const int n2 = dn.dense.n;
        // items a workgroup of the dense kernel stages at once and its operand images (dense_images::geometry, which the launcher
        // fills its launch from too); 256 bytes stand for the kernel's padding and zero words
        const dense_images::Geometry g = dense_images::geometry(fam, n2, int(elem));
        const int ipb = g.items;
        const size_t scratch = size_t(ipb) * size_t(ll + rl + 1) * elem;
        const size_t images = size_t(ipb) * (size_t(g.images) << n2) * elem + 256;
        if (scratch > 48 * 1024 || images + scratch > kLdsBytes - 1024 || w.list.row_out.size() > 32768) continue;
        // rows of the list -> components of the dense step's left image
        std::vector<int32_t> map_of(size_t(row_len(buf)), -1);
        for (size_t c = 0; c < dn.dense.left_map.size(); ++c) map_of[dn.dense.left_map[c] & 0xffffu] = int32_t(c);
        dn.pre.row_map.clear();
        dn.pre.row_scale.clear();
        bool covered = true;
        std::vector<uint32_t> row_start(1, 0u), entries;
        std::vector<double> coeff;
        std::vector<char> produced(dn.dense.left_map.size(), 0);
        for (size_t row = 0; row < w.list.row_out.size(); ++row) {
            const int32_t c = map_of[w.list.row_out[row]];
            if (c < 0) continue;   // a component the dense product does not read (its grade is not wanted there)
            produced[size_t(c)] = 1;
            dn.pre.row_map.push_back(dn.dense.left_map[size_t(c)] & 0xffff0000u);
            if (dn.dense.scaled) dn.pre.row_scale.push_back(dn.dense.left_scale[size_t(c)]);
            for (uint32_t e = w.list.row_start[row]; e < w.list.row_start[row + 1]; ++e) {
                entries.push_back(w.list.entries[e]);
                coeff.push_back(w.list.coeff[e]);
            }
            row_start.push_back(uint32_t(entries.size()));
        }
        for (char c : produced) covered = covered && c;
        // rows of one length with +-1 coefficients (R X: n entries per row): [term][row] words, sign in bit 31
        {
            const size_t rows = row_start.size() - 1;
            const uint32_t width = rows ? row_start[1] - row_start[0] : 0;
            bool uniform = rows > 0 && width > 0;
            for (size_t r = 0; uniform && r < rows; ++r) uniform = row_start[r + 1] - row_start[r] == width;
            for (size_t e = 0; uniform && e < coeff.size(); ++e) uniform = coeff[e] == 1.0 || coeff[e] == -1.0;
            for (size_t e = 0; uniform && e < entries.size(); ++e) uniform = (entries[e] & 0xffffu) < 0x8000u && (entries[e] >> 16) < 0x8000u;
            uniform = uniform && ll + rl + 1 < 0x8000;
            if (uniform) {
                // padded to a multiple of 4 terms with entries over the zero pair the kernel keeps behind the two rows
                // (left offset ll + rl from the left row, right offset rl from the right row): acc + (+0.0) changes no acc
                const uint32_t wpad = (width + 3u) & ~3u;
                const uint32_t zero_entry = uint32_t(ll + rl) | (uint32_t(rl) << 16);
                std::vector<uint32_t> ell(size_t(wpad) * rows, zero_entry);
                for (size_t r = 0; r < rows; ++r)
                    for (uint32_t t = 0; t < width; ++t) {
                        const size_t e = size_t(row_start[r]) + t;
                        ell[size_t(t) * rows + r] = entries[e] | (coeff[e] < 0.0 ? 0x80000000u : 0u);
                    }
                entries.swap(ell);
                coeff.clear();
                dn.pre.width = int(wpad);
            }
        }
        dn.dense.chained = 1;
        dn.pre.a = w.a;
        dn.pre.b = w.b;
        dn.pre.canon_a = w.canon_a;
        dn.pre.canon_b = w.canon_b;
        dn.pre.row_start = std::move(row_start);
        dn.pre.entries = std::move(entries);
        dn.pre.coeff = std::move(coeff);
        dn.pre.left_len = int(ll);
        dn.pre.right_len = int(rl);
        // components no row produces stay zero: the kernel zero-fills the image first unless every loaded component is covered
        dn.dense.left_full = dn.dense.left_full && covered;
        dn.dense.left_contig = 0;   // general staging
        dn.name += " <- " + w.name + " in LDS";
        dn.n_entries += w.n_entries;
        dn.a = BufRef{BufKind::NODE, -1};
        plan.node_dead[size_t(buf.idx)] = 1;
        w.kind = Step::ZERO;   // marks the list step for removal below
        w.res = BufRef{BufKind::NODE, -1};
    }
    std::vector<Step> kept;
    for (Step& t : plan.steps)
        if (!(t.kind == Step::ZERO && t.res.kind == BufKind::NODE && t.res.idx < 0)) kept.push_back(std::move(t));
    plan.steps = std::move(kept);
}

// A list product whose result is read ONLY by another list product (as either operand): both run in ONE k_product_ell_chain
// launch with the mid row in LDS -- the rotor sandwich applied to a vector, (R X ~R).g(1), where it no longer fits a fused
// small-program kernel (n >= 9) and its second product (n rows of 2^(n-1) terms) is far too sparse for the dense kernels.  Same
// order, same roundings: bit for bit the two-launch plan.  Off with GAAST_FLAG_DEBUG_NO_CHAIN.
static void chain_list_into_list(Plan& plan) {
    if (plan.flags & (GAAST_FLAG_NO_FUSION | GAAST_FLAG_DEBUG_NO_CHAIN)) return;
    if (plan.node_dead.size() != plan.node_buffers.size()) plan.node_dead.assign(plan.node_buffers.size(), 0);
    const size_t elem = plan.dtype == GAAST_F32 ? 4 : 8;
    auto row_len = [&](BufRef r) -> int64_t {
        return r.kind == BufKind::NODE ? plan.node_buffers[size_t(r.idx)].row_len : r.kind == BufKind::INPUT ? plan.input_layouts[size_t(r.idx)].row_len
                                                                                                           : plan.out_layout.row_len;
    };
    for (const Step& t : plan.steps)
        if (t.kind == Step::FUSED) return;
    for (size_t j = 0; j < plan.steps.size(); ++j) {
        Step& c = plan.steps[j];
        if (c.kind != Step::PRODUCT_CSR || c.list.ell_width <= 0 || !c.list.ell_bytes || c.chain.side) continue;
        for (int side = 1; side <= 2 && !c.chain.side; ++side) {
            const BufRef buf = side == 1 ? c.a : c.b, other = side == 1 ? c.b : c.a;
            if (buf.kind != BufKind::NODE || buf.idx < 0 || buf == other) continue;
            int writer = -1;
            bool ok = true;
            for (size_t i = 0; i < plan.steps.size() && ok; ++i) {
                const Step& t = plan.steps[i];
                if (i == j) continue;
                if (t.res == buf) {
                    if (writer >= 0 || t.kind != Step::PRODUCT_CSR || t.list.ell_width <= 0 || !t.list.ell_bytes || t.beta != 0 || t.chain.side || i > j) ok = false;
                    writer = int(i);
                }
                if (reads(t, buf)) ok = false;
            }
            if (!ok || writer < 0) continue;
            Step& w = plan.steps[size_t(writer)];
            if (w.a == buf || w.b == buf || c.res == w.a || c.res == w.b) continue;
            for (size_t i = size_t(writer) + 1; i < j && ok; ++i)
                if (plan.steps[i].res == w.a || plan.steps[i].res == w.b) ok = false;
            if (!ok) continue;
            const int64_t l1 = row_len(w.a), r1 = row_len(w.b), mid = row_len(buf), r2 = row_len(other);
            const int canon_other = side == 1 ? c.canon_b : c.canon_a;
            int alias = 0;
            if (other == w.a && canon_other == w.canon_a) alias = 1;
            else if (other == w.b && canon_other == w.canon_b) alias = 2;
            const int64_t per_item = l1 + r1 + mid + (alias ? 0 : r2);
            if (per_item * int64_t(elem) >= 32768 * 3) continue;       // byte offsets of the entries stay below 32 KiB per row anyway
            int64_t stride = per_item;
            while (stride % 32 != 1) ++stride;                         // consecutive items: consecutive banks
            // items per workgroup: about 36 KiB of LDS (four workgroups per CU: one's staging overlaps another's lists), at least
            // four items when that still fits the CU
            // this list's words ride in LDS when they take at most 48 KiB (n <= 11 for the sandwich)
            int64_t ent2 = ((int64_t(c.list.ell_width) + 4) * int64_t(c.list.row_out.size()) * 4 + 15) / 16 * 16;   // [row][term], rows 4 words apart; widths are multiples of 4
            if (ent2 > 48 * 1024 || c.list.ell_width % 4) ent2 = 0;
            // items per workgroup: as many as make this list's (row, item) pairs just fill a wave (9 rows: 7 items = 63 lanes) -- a
            // second, nearly empty wave would issue the whole list again --, fewer when the LDS does not hold them
            const int64_t rows2 = int64_t(c.list.row_out.size());
            int64_t ipb = rows2 <= 32 ? 64 / rows2 : 4;
            const int64_t lds_cap = int64_t(kLdsBytes) - 16 * 1024;
            while (ipb > 2 && ent2 + ipb * stride * int64_t(elem) > lds_cap / 2) --ipb;   // two workgroups per CU when that costs at most ...
            if (ipb < 4) {                                                                 // ... down to four items; then one workgroup per CU
                ipb = std::min<int64_t>(rows2 <= 32 ? 64 / rows2 : 4, 4);
                if (ent2 + ipb * stride * int64_t(elem) > lds_cap) ent2 = 0;
                while (ipb > 1 && ipb * stride * int64_t(elem) > lds_cap) --ipb;
            }
            if (ipb < 2 || ent2 + ipb * stride * int64_t(elem) > lds_cap) continue;
            c.chain.ent2_lds = int(ent2);
            // rows of the first list -> their element offsets in the mid row; is every component of the mid row produced?
            std::vector<char> produced(size_t(mid), 0);
            for (uint32_t off : w.list.row_out) produced[off] = 1;
            bool covered = true;
            for (char x : produced) covered = covered && x;
            c.chain.side = side;
            c.chain.alias = alias;
            c.chain.mid_len = int(mid);
            c.chain.canon_mid = side == 1 ? c.canon_a : c.canon_b;
            c.chain.covered = covered ? 1 : 0;
            c.chain.ipb = int(ipb);
            c.chain.item_stride = int(stride);
            c.pre.a = w.a;
            c.pre.b = w.b;
            c.pre.canon_a = w.canon_a;
            c.pre.canon_b = w.canon_b;
            c.pre.left_len = int(l1);
            c.pre.right_len = int(r1);
            c.pre.entries = w.list.entries;
            c.pre.row_map = w.list.row_out;
            c.pre.width = w.list.ell_width;
            c.name += " <- " + w.name + " in LDS";
            c.n_entries += w.n_entries;
            make_chain_jit(plan, c, &w, l1, r1, mid, r2, alias, side, covered);
            (side == 1 ? c.a : c.b) = BufRef{BufKind::NODE, -1};
            plan.node_dead[size_t(buf.idx)] = 1;
            w.kind = Step::ZERO;   // marks the first list for removal below
            w.res = BufRef{BufKind::NODE, -1};
        }
    }
    std::vector<Step> kept;
    for (Step& t : plan.steps)
        if (!(t.kind == Step::ZERO && t.res.kind == BufKind::NODE && t.res.idx < 0)) kept.push_back(std::move(t));
    plan.steps = std::move(kept);
}

// A RUN of element-wise arms on one buffer -- add_grades_from copies / additions of bound inputs, Negation / Reverse / GradeInvolution
// sign flips (eval.rs:45-60, 87-102) -- costs one full read-modify-write of the buffer PER ARM when every arm is a launch
// ((-(a.rev()) + b.ginvol()).rev() * s at n = 12: six passes).  The components never look at each other, so the run becomes ONE
// k_elementwise pass in which each component executes its own statements in program order: bit-identical.  When the run's buffer is
// only the operand of a product of one-term rows with a scalar operand, that product rides along as the pass's epilogue and the
// buffer is never written at all.
static void fuse_elementwise_runs(Plan& plan) {
    if (plan.flags & (GAAST_FLAG_NO_FUSION | GAAST_FLAG_DEBUG_NO_CHAIN)) return;
    auto row_len = [&](BufRef r) -> int64_t {
        return r.kind == BufKind::NODE ? plan.node_buffers[size_t(r.idx)].row_len : r.kind == BufKind::INPUT ? plan.input_layouts[size_t(r.idx)].row_len
                                                                                                           : plan.out_layout.row_len;
    };
    for (size_t i = 0; i < plan.steps.size(); ++i) {
        const Step& first = plan.steps[i];
        if (first.kind != Step::AXPY && first.kind != Step::FLIP && first.kind != Step::DUAL) continue;
        const BufRef R = first.res;
        size_t j = i;
        std::vector<BufRef> srcs;
        bool ok = true;
        while (j < plan.steps.size() && ok) {
            const Step& t = plan.steps[j];
            if ((t.kind != Step::AXPY && t.kind != Step::FLIP && t.kind != Step::DUAL) || t.res != R) break;
            if (t.kind != Step::FLIP) {   // AXPY, DUAL: statements that read a bound input
                if (t.a.kind != BufKind::INPUT) break;
                bool known = false;
                for (const BufRef& b : srcs) known = known || b == t.a;
                if (!known) {
                    if (srcs.size() == 6) break;
                    srcs.push_back(t.a);
                }
            }
            ++j;
            if (j - i == 8) break;   // (a pass holds eight statements per component; a longer run continues in a second pass)
        }
        const size_t n_ops = j - i;
        if (n_ops < 2) continue;
        // components the run touches, in row order
        const int64_t rl = row_len(R);
        std::vector<int32_t> comp_of(size_t(rl), -1);
        std::vector<uint32_t> comps;
        for (size_t k = i; k < j; ++k) {
            for (uint32_t w : plan.steps[k].axpy_map) comp_of[w & 0xffffu] = 0;
            for (uint32_t off : plan.steps[k].flip_offsets) comp_of[off] = 0;
            if (plan.steps[k].kind == Step::DUAL) plan.steps[k].dual.for_each([&](uint32_t r, uint32_t, bool) { comp_of[r] = 0; });
        }
        for (int64_t o = 0; o < rl; ++o)
            if (comp_of[size_t(o)] == 0) {
                comp_of[size_t(o)] = int32_t(comps.size());
                comps.push_back(uint32_t(o));
            }
        const size_t nc = comps.size();
        if (nc == 0) continue;
        std::vector<uint32_t> ops(n_ops * nc, 0u);
        for (size_t k = i; k < j; ++k) {
            const Step& t = plan.steps[k];
            if (t.kind == Step::FLIP) {
                for (uint32_t off : t.flip_offsets) ops[(k - i) * nc + size_t(comp_of[off])] = 2u;
            } else {
                uint32_t slot = 0;
                for (size_t q = 0; q < srcs.size(); ++q)
                    if (srcs[q] == t.a) slot = uint32_t(q);
                for (uint32_t w : t.axpy_map) ops[(k - i) * nc + size_t(comp_of[w & 0xffffu])] = (t.beta ? 1u : 3u) | (slot << 2) | ((w >> 16) << 16);
                if (t.kind == Step::DUAL)   // a complement: the same statement with the source negated (bit 5) and read as a product operand (bit 6)
                    t.dual.for_each([&](uint32_t r, uint32_t a, bool neg) {
                        ops[(k - i) * nc + size_t(comp_of[r])] = (t.beta ? 1u : 3u) | (slot << 2) | (neg ? 32u : 0u) | (t.canon_a ? 64u : 0u) | (a << 16);
                    });
            }
        }
        // Every component executes ITS OWN statements in order, so each list is compacted on its own: empty statements go, and two
        // sign flips in a row cancel exactly (-(-x) has the bits of x) -- (-(a.rev()) + b.ginvol()).rev() on grade-6 rows is
        // copy, flip, flip, add, flip: three statements.  Four or fewer statements run on the kernel instantiation with half the
        // registers (k_elementwise<T, 4>).
        {
            std::vector<std::vector<uint32_t>> lists(nc);
            size_t longest = 1;
            for (size_t c = 0; c < nc; ++c) {
                for (size_t k = 0; k < n_ops; ++k) {
                    const uint32_t w = ops[k * nc + c];
                    if ((w & 3u) == 0u) continue;
                    if ((w & 3u) == 2u && !lists[c].empty() && (lists[c].back() & 3u) == 2u) lists[c].pop_back();
                    else lists[c].push_back(w);
                }
                longest = std::max(longest, lists[c].size());
            }
            ops.assign(longest * nc, 0u);
            for (size_t c = 0; c < nc; ++c)
                for (size_t k = 0; k < lists[c].size(); ++k) ops[k * nc + c] = lists[c][k];
        }
        const size_t n_stmt = ops.size() / nc;
        // does every component start with a copy (the run then never reads its buffer)?
        bool load_first = false;
        for (size_t c = 0; c < nc && !load_first; ++c) {
            size_t k = 0;
            while (k < n_stmt && ops[k * nc + c] == 0u) ++k;
            load_first = k == n_stmt || (ops[k * nc + c] & 3u) != 3u;
        }
        Step f;
        f.kind = Step::ELEMENTWISE;
        f.res = R;
        f.ew.src = srcs;
        f.ew.n_ops = int(n_stmt);
        f.ew.load_first = load_first ? 1 : 0;
        f.ew.ops = std::move(ops);
        f.ew.comp_off = comps;
        f.name = "elementwise[" + std::to_string(n_ops) + " arms:";
        for (size_t k = i; k < j; ++k) f.name += " " + plan.steps[k].name.substr(0, plan.steps[k].name.find('[') == std::string::npos ? 8 : plan.steps[k].name.find('['));
        f.name += "]";
        // the scaling product right after the run, reading the run's buffer and a scalar?
        size_t drop_to = j;
        if (R.kind == BufKind::NODE && j < plan.steps.size() && !load_first && int64_t(nc) == rl) {
            const Step& p2 = plan.steps[j];
            const bool r_left = p2.kind == Step::PRODUCT_CSR && p2.a == R, r_right = p2.kind == Step::PRODUCT_CSR && p2.b == R;
            if (p2.kind == Step::PRODUCT_CSR && p2.beta == 0 && r_left != r_right && !p2.chain.side && p2.list.row_out.size() == nc) {
                const BufRef S = r_left ? p2.b : p2.a;
                bool fits = row_len(S) == 1 && S != R && p2.res != R;
                for (size_t r = 0; r + 1 < p2.list.row_start.size() && fits; ++r) fits = p2.list.row_start[r + 1] - p2.list.row_start[r] == 1;
                for (size_t k = 0; k < plan.steps.size() && fits; ++k) {   // nobody else reads the run's buffer
                    if (k >= i && k <= j) continue;
                    const Step& t = plan.steps[k];
                    if (t.res == R || reads(t, R)) fits = false;
                }
                std::vector<uint32_t> out_off(nc, 0u);
                std::vector<double> coeff(nc, 0.0);
                std::vector<char> seen(nc, 0);
                for (size_t r = 0; r + 1 < p2.list.row_start.size() && fits; ++r) {
                    const uint32_t e = p2.list.entries[p2.list.row_start[r]];
                    const uint32_t roff = r_left ? (e & 0xffffu) : (e >> 16);
                    fits = roff < uint32_t(rl) && comp_of[roff] >= 0 && !seen[size_t(comp_of[roff])];
                    if (!fits) break;
                    seen[size_t(comp_of[roff])] = 1;
                    out_off[size_t(comp_of[roff])] = p2.list.row_out[r];
                    coeff[size_t(comp_of[roff])] = p2.list.coeff[p2.list.row_start[r]];
                }
                if (fits) {
                    f.ew.scale = 1;
                    f.res = p2.res;
                    f.b = S;
                    f.ew.out_off = std::move(out_off);
                    f.ew.coeff = std::move(coeff);
                    f.ew.scalar_off = 0;
                    f.ew.canon_v = r_left ? p2.canon_a : p2.canon_b;
                    f.ew.canon_s = r_left ? p2.canon_b : p2.canon_a;
                    f.ew.s_is_left = r_left ? 0 : 1;
                    f.beta = 0;
                    f.n_entries = p2.n_entries;
                    f.name += " * scalar -> " + p2.name;
                    if (plan.node_dead.size() != plan.node_buffers.size()) plan.node_dead.assign(plan.node_buffers.size(), 0);
                    plan.node_dead[size_t(R.idx)] = 1;
                    drop_to = j + 1;
                }
            }
        }
        std::vector<Step> kept;
        for (size_t k = 0; k < plan.steps.size(); ++k) {
            if (k == i) kept.push_back(std::move(f));
            else if (k > i && k < drop_to) continue;
            else kept.push_back(std::move(plan.steps[k]));
        }
        plan.steps = std::move(kept);
    }
}

// x (*) f(<l, r>): a product into ONE scalar component (a single row: norm_sq), an optional ScalarUnaryOp on it, and a product of
// one-term rows that multiplies another row by that scalar -- a.rev() * a.norm_sq().sinv(), the versor inverse of expr.rs:363-371,
// where the rows no longer fit a fused slab -- become ONE k_reduce_scale launch (kernels_exact.hip.hpp): reference order and
// roundings, the scalar never leaves the wave, the row is streamed once from HBM.  Runs on the CSR form, before the ELL pass.
static void fuse_reduce_scale(Plan& plan) {
    if (plan.flags & (GAAST_FLAG_NO_FUSION | GAAST_FLAG_DEBUG_NO_CHAIN)) return;
    for (size_t i = 0; i + 1 < plan.steps.size(); ++i) {
        Step& p1 = plan.steps[i];
        if (p1.kind != Step::PRODUCT_CSR || p1.list.row_out.size() != 1 || p1.beta != 0 || p1.res.kind != BufKind::NODE || p1.chain.side) continue;
        if (plan.node_buffers[size_t(p1.res.idx)].row_len != 1 || p1.list.entries.size() < 64) continue;
        const BufRef S = p1.res;
        size_t j = i + 1;
        int op = 0;
        if (plan.steps[j].kind == Step::SUNARY && plan.steps[j].res == S && plan.steps[j].sunary_off == 0) {
            op = plan.steps[j].sunary_op == 0 ? 1 : 2;
            ++j;
        }
        if (j >= plan.steps.size()) continue;
        Step& p2 = plan.steps[j];
        if (p2.kind != Step::PRODUCT_CSR || p2.beta != 0 || p2.chain.side) continue;
        const bool s_left = p2.a == S, s_right = p2.b == S;
        if (s_left == s_right) continue;
        const BufRef xop = s_left ? p2.b : p2.a;
        if (xop == S || p2.res == p1.a || p2.res == p1.b || p2.res == xop) continue;
        bool ok = true;
        for (size_t r = 0; r + 1 < p2.list.row_start.size() && ok; ++r) ok = p2.list.row_start[r + 1] - p2.list.row_start[r] == 1;   // one term per row
        for (size_t k = 0; k < plan.steps.size() && ok; ++k) {   // nobody else touches the scalar
            if (k == i || k == j || (op && k == i + 1)) continue;
            const Step& t = plan.steps[k];
            if (t.res == S || reads(t, S)) ok = false;
        }
        if (!ok) continue;
        Step f;
        f.kind = Step::REDUCE_SCALE;
        f.res = p2.res;
        f.a = p1.a;
        f.b = p1.b;
        f.reduce.x = xop;
        f.canon_a = p1.canon_a;
        f.canon_b = p1.canon_b;
        f.reduce.canon_x = s_left ? p2.canon_b : p2.canon_a;
        f.reduce.canon_s = s_left ? p2.canon_a : p2.canon_b;
        f.reduce.op = op;
        f.reduce.s_is_left = s_left ? 1 : 0;
        f.reduce.ent1 = p1.list.entries;
        f.reduce.coeff1 = p1.list.coeff;
        f.reduce.ent2.resize(p2.list.entries.size());
        f.reduce.coeff2 = p2.list.coeff;
        for (size_t r = 0; r + 1 < p2.list.row_start.size(); ++r) {
            const uint32_t e = p2.list.entries[p2.list.row_start[r]];
            const uint32_t xoff = s_left ? (e >> 16) : (e & 0xffffu);
            f.reduce.ent2[r] = xoff | (p2.list.row_out[r] << 16);
        }
        f.beta = 0;
        f.n_entries = p1.n_entries + p2.n_entries;
        // tolerance mode: can a wave keep the row in registers and read it once (k_reduce_scale_wave)?  The reduction must be one term
        // per component, (i, i), coefficient +-1, in any order; the scaling one row per component in place (x offset = out offset),
        // +-1; the row a whole number of 64 x 16 bytes with at most 32 components per lane.  (Whether the three rows ARE one row is
        // known when they are bound: run_reduce.)
        if (!(plan.flags & GAAST_FLAG_EXACT_ORDER) && p1.a == p1.b && xop == p1.a) {
            const size_t per_piece = 64 * (plan.dtype == GAAST_F32 ? 4 : 2);   // components a wave moves per 16-byte load
            const Step::Reduce& q = f.reduce;
            const size_t R = q.ent1.size();
            bool okw = R == q.ent2.size() && R % per_piece == 0 && (R / per_piece) * (per_piece / 64) <= 32 && q.coeff1.size() == R && q.coeff2.size() == R;
            const size_t pieces = okw ? R / per_piece : 0;
            okw = okw && (pieces == 1 || pieces == 2 || pieces == 4 || pieces == 8 || pieces == 16);
            std::vector<uint32_t> sg(128, 0u);
            std::vector<char> seen1(R, 0), seen2(R, 0);
            const size_t ec = per_piece / 64;
            auto place = [&](size_t c, int which) {   // component c of the row -> (lane, bit)
                const size_t piece = c / ec, e = c % ec, m = piece / 64, lane = piece % 64;
                sg[size_t(which) * 64 + lane] |= 1u << (m * ec + e);
            };
            for (size_t t = 0; okw && t < R; ++t) {
                const uint32_t li = q.ent1[t] & 0xffffu, ri = q.ent1[t] >> 16;
                okw = li == ri && li < R && !seen1[li] && (q.coeff1[t] == 1.0 || q.coeff1[t] == -1.0);
                if (okw) {
                    seen1[li] = 1;
                    if (q.coeff1[t] < 0) place(li, 0);
                }
            }
            for (size_t r = 0; okw && r < R; ++r) {
                const uint32_t xo = q.ent2[r] & 0xffffu, oo = q.ent2[r] >> 16;
                okw = xo == oo && xo < R && !seen2[xo] && (q.coeff2[r] == 1.0 || q.coeff2[r] == -1.0);
                if (okw) {
                    seen2[xo] = 1;
                    if (q.coeff2[r] < 0) place(xo, 1);
                }
            }
            if (okw) {
                f.reduce.wave = int(pieces);
                f.reduce.sign_words = std::move(sg);
            }
        }
        f.name = "reduce_scale[" + std::to_string(p1.list.entries.size()) + " comp-muls -> scalar" + (op == 1 ? ", 1/s" : op == 2 ? ", sqrt(s)" : "") + ", " +
                 std::to_string(p2.list.entries.size()) + " scaled components]";
        if (plan.node_dead.size() != plan.node_buffers.size()) plan.node_dead.assign(plan.node_buffers.size(), 0);
        plan.node_dead[size_t(S.idx)] = 1;
        // out offsets need 16 bits
        bool fits = true;
        for (uint32_t o : p2.list.row_out) fits = fits && o < 65536u;
        if (!fits) continue;
        std::vector<Step> kept;
        for (size_t k = 0; k < plan.steps.size(); ++k) {
            if (k == i) kept.push_back(std::move(f));
            else if (k == j || (op && k == i + 1)) continue;
            else kept.push_back(std::move(plan.steps[k]));
        }
        plan.steps = std::move(kept);
        return fuse_reduce_scale(plan);   // (indices moved: look again for another instance)
    }
}

// A list with FEW LONG rows that stayed a launch of its own -- b * c projected on a low grade: (a + b * c).g(2) at n = 8 is 28 rows of 256
// terms -- gives k_product_ell (a thread per row) 28 busy threads per workgroup.  The specialised chain kernel's second list is exactly
// this shape (lane = (row, item), 32 items per workgroup): the list runs on it alone.  When the step before it is the covering copy of
// an input's grades into the same buffer (a + ...), that copy is folded in as well: the accumulators start from 0.0 + a -- ONE launch.
// Same order, same roundings; k_product_ell (and the copy) stay in charge when hiprtc is not available.
static void jit_long_row_lists(Plan& plan) {
    if (plan.flags & (GAAST_FLAG_NO_FUSION | GAAST_FLAG_NO_JIT | GAAST_FLAG_DEBUG_JIT_FAILS | GAAST_FLAG_DEBUG_NO_CHAIN)) return;
    auto row_len = [&](BufRef r) -> int64_t {
        return r.kind == BufKind::NODE ? plan.node_buffers[size_t(r.idx)].row_len : r.kind == BufKind::INPUT ? plan.input_layouts[size_t(r.idx)].row_len
                                                                                                           : plan.out_layout.row_len;
    };
    for (size_t j = 0; j < plan.steps.size(); ++j) {
        Step& c = plan.steps[j];
        if (c.kind != Step::PRODUCT_CSR || c.list.ell_width < 32 || !c.list.ell_bytes || c.chain.side || c.cj.on) continue;
        const int64_t rows = int64_t(c.list.row_out.size());
        if (rows > 128 || c.a.idx < 0 || c.b.idx < 0) continue;
        const int64_t la = row_len(c.a), lb = row_len(c.b);
        // the covering copy right before it, into the same buffer?
        std::vector<uint32_t> init;
        bool fold = false;
        if (j > 0 && c.beta == 1) {
            const Step& ax = plan.steps[j - 1];
            if (ax.kind == Step::AXPY && ax.beta == 0 && ax.res == c.res && ax.a.kind == BufKind::INPUT && int64_t(ax.axpy_map.size()) == rows) {
                std::vector<int64_t> src_of(size_t(row_len(c.res)), -1);
                for (uint32_t m : ax.axpy_map) src_of[m & 0xffffu] = int64_t(m >> 16);
                fold = true;
                for (int64_t r = 0; r < rows && fold; ++r) {
                    fold = src_of[c.list.row_out[size_t(r)]] >= 0;
                    init.push_back(uint32_t(fold ? src_of[c.list.row_out[size_t(r)]] : 0));
                }
            }
        }
        make_chain_jit(plan, c, nullptr, 0, 0, la, lb, 0, 1, true, fold ? &init : nullptr);
        if (!c.cj.on) continue;
        c.cj.single = 1;
        if (fold) {
            c.cj.fold_prev = 1;
            c.cj.init_src = plan.steps[j - 1].a;   // the copy's source: the accumulators' starting values
        }
    }
}

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
            if (!child_ok(nd.child0) || !child_ok(nd.child1)) throw std::runtime_error("nodes are not in post-order");
            if (nd.opcode == GAAST_OP_PRODUCT && nd.product_kind >= GAAST_PROD_ADJ_LEFT) {
                const int adj = nd.product_kind & ~7, base = nd.product_kind & 7;
                if ((adj != GAAST_PROD_ADJ_LEFT && adj != GAAST_PROD_ADJ_RIGHT) || base > GAAST_PROD_REGRESSIVE)
                    throw std::runtime_error("unknown product kind");
            }
            break;
        case GAAST_OP_NEG: case GAAST_OP_EXP: case GAAST_OP_LOG: case GAAST_OP_PROJ:
        case GAAST_OP_REVERSE: case GAAST_OP_GINVOL: case GAAST_OP_SINV: case GAAST_OP_SSQRT:
        case GAAST_OP_DUAL: case GAAST_OP_UNDUAL: case GAAST_OP_INV: case GAAST_OP_GEXP:
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
    if (!try_fuse(plan, small_reg_slab)) {
        fuse_elementwise_runs(plan);
        fuse_reduce_scale(plan);
        chain_sparse_into_dense(plan);
        uniform_csr_to_ell(plan);
        chain_list_into_list(plan);
        jit_long_row_lists(plan);
    }
}

}  // namespace gaast
