// Second order through the general exponential on the host, under AddressSanitizer + UBSan (CPU build only; no GPU, no HIP, never
// loaded into Python): gaast_program_vjp under GAAST_FLAG_GEXP_GRAD2 through the family {GEXP_ADJ, GEXP_JVP, GEXP_ADJ2} (host/vjp.cpp:
// gexp_family_adjoint, the third child in dep / keep / remap) and the lowering into Step::GEXP_JVP / Step::GEXP_ADJ2 (plan.cpp:
// lower_gexp2) under every plan form.  It also prints the tables of the lowered steps of hand-built programs ("G2OUT ..." /
// "G2TAB ..." lines) for tests/test_gexp2_host.py to compare with numpy.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "gaast_expr.h"
#include "plan.hpp"

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("CHECK failed: %s (line %d)\n", #c, __LINE__);  \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static std::vector<gaast_expr_t> handles;
static gaast_expr_t H(gaast_expr_t e) {
    handles.push_back(e);
    return e;
}

static int count_op(const gaast_program_desc& d, int opcode) {
    int c = 0;
    for (int i = 0; i < d.n_nodes; ++i) c += d.nodes[i].opcode == opcode;
    return c;
}
static int count_steps(const gaast::Plan& plan, gaast::Step::Kind k) {
    int c = 0;
    for (const gaast::Step& s : plan.steps) c += s.kind == k;
    return c;
}

// every table of a GEXP_JVP / GEXP_ADJ2 step has its size, every offset stays inside the row it indexes, no result component is written
// twice, and all three operand rows are in the one list of the step's reads
static void check_step(const gaast::Plan& plan, const gaast::Step& s) {
    const bool adj2 = s.kind == gaast::Step::GEXP_ADJ2;
    const gaast::Layout &la = plan.layout(s.a), &lr = plan.layout(s.res);
    const gaast::Step::Inverse& q = s.inv;
    CHECK(s.a.idx >= 0 && s.c.idx >= 0 && (s.b.idx >= 0) == adj2);
    CHECK(!(s.a == s.res) && !(s.c == s.res) && !(adj2 && s.b == s.res));
    CHECK(q.N == 2 || q.N == 4 || q.N == 8 || q.N == 16 || q.N == 32 || q.N == 64);
    CHECK(q.N == (1 << (q.even ? plan.n - 1 : plan.n)));
    CHECK(q.blade.size() == size_t(q.N) && q.a_off.size() == size_t(q.N) && q.res_off.size() == size_t(q.N) && q.neg.size() == size_t(q.N));
    CHECK(q.h_off.size() == size_t(q.N) && q.adj_neg_l.size() == size_t(q.N) && q.adj_neg_r.size() == size_t(q.N));
    CHECK(q.g_off.size() == (adj2 ? size_t(q.N) : size_t(0)));
    CHECK(q.weight.size() == size_t(1) << plan.n && q.weight.size() <= 128);
    double wmax = 0;
    for (double w : q.weight) wmax = std::fmax(wmax, std::fabs(w));
    CHECK(q.wmax == wmax);
    if (q.h_off.size() != size_t(q.N) || q.adj_neg_l.size() != size_t(q.N) || q.adj_neg_r.size() != size_t(q.N) || q.g_off.size() != (adj2 ? size_t(q.N) : size_t(0))) return;
    std::vector<char> seen(size_t(lr.row_len), 0);
    int produced = 0;
    for (int j = 0; j < q.N; ++j) {
        CHECK(q.a_off[size_t(j)] >= -1 && int64_t(q.a_off[size_t(j)]) < la.row_len);
        CHECK(q.res_off[size_t(j)] >= -1 && int64_t(q.res_off[size_t(j)]) < lr.row_len);
        CHECK(q.h_off[size_t(j)] >= -1 && int64_t(q.h_off[size_t(j)]) < plan.layout(s.c).row_len);
        if (adj2) CHECK(q.g_off[size_t(j)] >= -1 && int64_t(q.g_off[size_t(j)]) < plan.layout(s.b).row_len);
        if (q.res_off[size_t(j)] >= 0 && int64_t(q.res_off[size_t(j)]) < lr.row_len) {
            CHECK(!seen[size_t(q.res_off[size_t(j)])]);
            seen[size_t(q.res_off[size_t(j)])] = 1;
            ++produced;
            if (adj2) CHECK(q.a_off[size_t(j)] >= 0);   // the gradient is restricted to what the operand holds
        }
        for (int r = 0; r < q.N; ++r) {
            const uint64_t want = (q.neg[size_t(r ^ j)] >> j) & 1ULL;   // a = r, b = j: the sign of L[a xor b][b]
            CHECK(((q.adj_neg_l[size_t(r)] >> j) & 1ULL) == want && ((q.adj_neg_r[size_t(j)] >> r) & 1ULL) == want);
        }
    }
    CHECK(produced == q.n_out && produced > 0);
    if (s.beta == 0) CHECK(int64_t(produced) == lr.row_len);
    if (q.N < 64) CHECK((q.a_neg >> q.N) == 0);
    int hits = 0;
    gaast::for_each_read(s, [&](gaast::BufRef r) { hits += (r == s.a) + (r == s.c) + (adj2 && r == s.b); });
    CHECK(hits >= (adj2 ? 3 : 2));
}

static void print_steps(const gaast::Plan& plan, const char* tag) {
    for (const gaast::Step& s : plan.steps) {
        if (s.kind != gaast::Step::GEXP_JVP && s.kind != gaast::Step::GEXP_ADJ2) continue;
        const gaast::Step::Inverse& q = s.inv;
        const char* kind = s.kind == gaast::Step::GEXP_ADJ2 ? "adj2" : "jvp";
        for (int j = 0; j < q.N; ++j)
            std::printf("G2OUT %s %s %d %d %u %d %d %d %d %d %.17g\n", tag, kind, q.N, j, q.blade[size_t(j)], q.a_off[size_t(j)], q.res_off[size_t(j)],
                        q.g_off.empty() ? -2 : q.g_off[size_t(j)], q.h_off[size_t(j)], int((q.a_neg >> j) & 1), q.wmax);
        for (int a = 0; a < q.N; ++a)
            for (int b = 0; b < q.N; ++b) {
                const double w = q.weight[size_t(q.blade[size_t(a)] & q.blade[size_t(b)])];
                std::printf("G2TAB %s %s %d %d %.17g %.17g %.17g\n", tag, kind, a, b, q.coeff(a, b), ((q.adj_neg_l[size_t(a)] >> b) & 1ULL) ? -w : w,
                            ((q.adj_neg_r[size_t(b)] >> a) & 1ULL) ? -w : w);
            }
    }
}

// lowers `d` under every plan form: as many GEXP_JVP / GEXP_ADJ2 steps as nodes (at least: a node under a sign-only arm is evaluated
// once per buffer it is added into), each a launch of its own, none of them owning the domain-error counter
static void lower_all(const gaast_program_desc& d, const char* what, const char* tab = nullptr) {
    const int n_jvp = count_op(d, GAAST_OP_GEXP_JVP), n_adj2 = count_op(d, GAAST_OP_GEXP_ADJ2);
    for (uint32_t extra : {0u, uint32_t(GAAST_FLAG_NO_FUSION), uint32_t(GAAST_FLAG_NO_JIT), uint32_t(GAAST_FLAG_EXACT_ORDER), uint32_t(GAAST_FLAG_DEBUG_JIT_FAILS)}) {
        gaast_program_desc b = d;
        b.flags |= extra;
        gaast::Plan plan;
        gaast::build_plan(b, plan);
        if (plan.error != GAAST_OK) std::printf("%s: plan error %d: %s\n", what, plan.error, plan.error_msg.c_str());
        CHECK(plan.error == GAAST_OK);
        if (!plan.unsupported.empty()) std::printf("%s: unsupported: %s\n", what, plan.unsupported.c_str());
        CHECK(plan.unsupported.empty());
        CHECK(count_steps(plan, gaast::Step::GEXP_JVP) >= n_jvp && count_steps(plan, gaast::Step::GEXP_ADJ2) >= n_adj2);
        CHECK((n_jvp > 0) == (count_steps(plan, gaast::Step::GEXP_JVP) > 0) && (n_adj2 > 0) == (count_steps(plan, gaast::Step::GEXP_ADJ2) > 0));
        CHECK(plan.has_gexp == (count_steps(plan, gaast::Step::GEXP) > 0));
        CHECK(count_steps(plan, gaast::Step::FUSED) == 0 || n_jvp + n_adj2 == 0);
        for (const gaast::Step& s : plan.steps)
            if (s.kind == gaast::Step::GEXP_JVP || s.kind == gaast::Step::GEXP_ADJ2) check_step(plan, s);
        if (tab && extra == 0) print_steps(plan, tab);
    }
}

static void round_trip(const gaast_program_desc& a) {
    const size_t need = gaast_program_serialize(&a, nullptr, 0);
    std::vector<unsigned char> buf(need);
    CHECK(gaast_program_serialize(&a, buf.data(), need) == need);
    gaast_program_image_t img = gaast_program_deserialize(buf.data(), need);
    CHECK(img != nullptr);
    if (!img) return;
    const gaast_program_desc& b = *gaast_program_image_desc(img);
    CHECK(b.n_nodes == a.n_nodes && b.root == a.root && b.flags == a.flags);
    for (int i = 0; i < a.n_nodes && i < b.n_nodes; ++i)
        CHECK(a.nodes[i].opcode == b.nodes[i].opcode && a.nodes[i].child0 == b.nodes[i].child0 && a.nodes[i].child1 == b.nodes[i].child1 &&
              a.nodes[i].input_slot == b.nodes[i].input_slot && a.nodes[i].minimal_grade_mask == b.nodes[i].minimal_grade_mask);
    gaast_program_image_free(img);
}

// the node shapes of the table in gaast_expr.h, in any image
static void check_family_nodes(const gaast_program_desc& a) {
    for (int i = 0; i < a.n_nodes; ++i) {
        const gaast_node_desc& nd = a.nodes[i];
        if (nd.opcode == GAAST_OP_GEXP_JVP) {
            CHECK(nd.child0 >= 0 && nd.child0 < i && nd.child1 >= 0 && nd.child1 < i);
            if (nd.child0 >= 0 && nd.child1 >= 0) CHECK((a.nodes[nd.child0].minimal_grade_mask & ~a.nodes[nd.child1].minimal_grade_mask) == 0);
        } else if (nd.opcode == GAAST_OP_GEXP_ADJ2) {
            CHECK(nd.child0 >= 0 && nd.child0 < i && nd.child1 >= 0 && nd.child1 < i && nd.input_slot >= 0 && nd.input_slot < i);
            if (nd.child1 >= 0 && nd.input_slot >= 0 && nd.input_slot < i) {
                CHECK((a.nodes[nd.child1].minimal_grade_mask & ~a.nodes[nd.input_slot].minimal_grade_mask) == 0);
                CHECK(nd.minimal_grade_mask == a.nodes[nd.input_slot].minimal_grade_mask);
            }
        }
    }
}

// first order in every batched slot, then second order in every batched slot of each image, lowered under every plan form; the third
// order is refused by name exactly where a GEXP_ADJ2 node is on the path
static void exercise(gaast_expr_t e, int n, const double* metric, const char* what) {
    gaast_spec_t spec = gaast_expr_specialize(e, n, metric, 0);
    CHECK(spec != nullptr);
    if (!spec) return;
    int seen_jvp = 0, seen_adj2 = 0, refused3 = 0;
    for (int dtype : {GAAST_F64, GAAST_F32}) {
        gaast_program_desc desc;
        CHECK(gaast_spec_program_desc(spec, dtype, GAAST_FLAG_GEXP_GRAD2, &desc) == 0);
        for (int s1 = 0; s1 < desc.n_inputs; ++s1) {
            if (desc.inputs[s1].is_const) continue;
            gaast_program_image_t i1 = nullptr;
            CHECK(gaast_program_vjp(&desc, s1, &i1) == 0 && i1);
            if (!i1) continue;
            const gaast_program_desc& a = *gaast_program_image_desc(i1);
            CHECK(a.flags == desc.flags && count_op(a, GAAST_OP_GEXP_JVP) == 0 && count_op(a, GAAST_OP_GEXP_ADJ2) == 0);
            for (int s2 = 0; s2 < a.n_inputs; ++s2) {
                if (a.inputs[s2].is_const) continue;
                gaast_program_image_t i2 = nullptr;
                const int st = gaast_program_vjp(&a, s2, &i2);
                if (st) std::printf("%s: second order (%d, %d): status %d: %s\n", what, s1, s2, st, gaast_expr_last_error());
                CHECK(st == 0 && i2);
                if (!i2) continue;
                const gaast_program_desc& a2 = *gaast_program_image_desc(i2);
                seen_jvp += count_op(a2, GAAST_OP_GEXP_JVP);
                seen_adj2 += count_op(a2, GAAST_OP_GEXP_ADJ2);
                check_family_nodes(a2);
                lower_all(a2, what);
                round_trip(a2);
                for (int s3 = 0; s3 < a2.n_inputs; ++s3) {   // third order: closed for JVP / ADJ nodes, refused through ADJ2
                    if (a2.inputs[s3].is_const) continue;
                    gaast_program_image_t i3 = nullptr;
                    const int st3 = gaast_program_vjp(&a2, s3, &i3);
                    if (st3) {
                        CHECK(st3 == GAAST_ERR_UNIMPLEMENTED && std::strstr(gaast_expr_last_error(), "third-order reverse mode through GAAST_OP_GEXP_ADJ2") != nullptr);
                        CHECK(count_op(a2, GAAST_OP_GEXP_ADJ2) > 0);
                        ++refused3;
                    } else if (i3) {
                        check_family_nodes(*gaast_program_image_desc(i3));
                        if (dtype == GAAST_F64) lower_all(*gaast_program_image_desc(i3), what);
                        gaast_program_image_free(i3);
                    }
                }
                gaast_program_image_free(i2);
            }
            gaast_program_image_free(i1);
        }
    }
    CHECK(seen_jvp > 0 && seen_adj2 > 0 && refused3 > 0);
    gaast_spec_free(spec);
    std::printf("ok  %s\n", what);
}

struct Raw {
    std::vector<gaast_node_desc> nodes;
    std::vector<gaast_input_desc> ins;
    gaast_program_desc d{};
    int input(uint64_t mask, int n) {
        gaast_node_desc nd{};
        nd.opcode = GAAST_OP_INPUT; nd.child0 = nd.child1 = -1; nd.input_slot = int(ins.size()); nd.minimal_grade_mask = mask; nd.vec_space_dim = n;
        nd.product_kind = GAAST_PROD_EXPLICIT;
        ins.push_back(gaast_input_desc{mask, n, 0, nullptr});
        nodes.push_back(nd);
        return int(nodes.size()) - 1;
    }
    int node(int opcode, int c0, int c1, int third, uint64_t mask, int n) {
        gaast_node_desc nd{};
        nd.opcode = opcode; nd.child0 = c0; nd.child1 = c1; nd.input_slot = third; nd.minimal_grade_mask = mask; nd.vec_space_dim = n;
        nd.product_kind = GAAST_PROD_EXPLICIT;
        nodes.push_back(nd);
        return int(nodes.size()) - 1;
    }
    const gaast_program_desc& desc(int n, const double* metric) {
        d.vec_space_dim = n; d.metric_diag = metric; d.dtype = GAAST_F64; d.n_inputs = int(ins.size()); d.inputs = ins.data();
        d.n_nodes = int(nodes.size()); d.nodes = nodes.data(); d.root = d.n_nodes - 1;
        return d;
    }
};

int main() {
    const double pga[4] = {0, 1, 1, 1}, ones[GAAST_MAX_DIM > 8 ? GAAST_MAX_DIM : 8] = {1, 1, 1, 1, 1, 1, 1, 1};
    {
        gaast_expr_t x = H(gaast_expr_input(0, 0x5, 3)), y = H(gaast_expr_input(1, 0x5, 3));
        exercise(H(gaast_expr_product(H(gaast_expr_gexp(x)), y, GAAST_PROD_GEOMETRIC)), 3, ones, "gexp(x) * y");
        gaast_expr_t B = H(gaast_expr_input(0, 0x4, 4)), X = H(gaast_expr_input(1, 0x8, 4));
        gaast_expr_t R = H(gaast_expr_gexp(B));
        exercise(H(gaast_expr_product(H(gaast_expr_product(R, X, GAAST_PROD_GEOMETRIC)), H(gaast_expr_rev(R)), GAAST_PROD_GEOMETRIC)), 4, pga, "gexp(B) X ~gexp(B)");
        exercise(H(gaast_expr_product(H(gaast_expr_gexp(H(gaast_expr_rev(B)))), X, GAAST_PROD_GEOMETRIC)), 4, pga, "gexp(~B) X");
    }
    {   // the tables the host test compares with numpy.  PGA3D even: every operand holds the even grades
        Raw j;
        const int h = j.input(0x15, 4), a = j.input(0x15, 4);
        j.node(GAAST_OP_GEXP_JVP, h, a, -1, 0x15, 4);
        lower_all(j.desc(4, pga), "raw jvp, PGA3D even", "pga-even");
        round_trip(j.d);
        Raw k;
        const int g = k.input(0x15, 4), h2 = k.input(0x15, 4), a2 = k.input(0x15, 4);
        k.node(GAAST_OP_GEXP_ADJ2, g, h2, a2, 0x15, 4);
        lower_all(k.desc(4, pga), "raw adj2, PGA3D even", "pga-even");
        round_trip(k.d);
        // absent and wanted grades, a folded sign: A = ~B a bivector (grade 2 negated in the read), h a bivector, g without grade 4, the
        // tangent's result wanted in grades 2 and 4 only
        Raw p;
        const int hp = p.input(0x4, 4), bp = p.input(0x4, 4);
        const int ap = p.node(GAAST_OP_REVERSE, bp, -1, -1, 0x4, 4);
        p.node(GAAST_OP_GEXP_JVP, hp, ap, -1, 0x14, 4);
        lower_all(p.desc(4, pga), "raw jvp, PGA3D parts", "pga-part");
        Raw r;
        const int gr = r.input(0x5, 4), hr = r.input(0x4, 4), br = r.input(0x4, 4);
        const int ar = r.node(GAAST_OP_REVERSE, br, -1, -1, 0x4, 4);
        r.node(GAAST_OP_GEXP_ADJ2, gr, hr, ar, 0x4, 4);
        lower_all(r.desc(4, pga), "raw adj2, PGA3D parts", "pga-part");
        round_trip(r.d);
        std::printf("ok  raw tables\n");
    }
    {   // malformed nodes of the raw ABI are refused, not read out of bounds
        Raw j;   // a tangent with a grade the operand lacks
        const int h = j.input(0x5, 3), a = j.input(0x4, 3);
        j.node(GAAST_OP_GEXP_JVP, h, a, -1, 0x5, 3);
        gaast::Plan plan;
        gaast::build_plan(j.desc(3, ones), plan);
        CHECK(plan.error == GAAST_ERR_INVALID_PROGRAM);
        Raw k;   // a cotangent outside the blade set
        const int g = k.input(0x2, 3), h2 = k.input(0x4, 3), a2 = k.input(0x4, 3);
        k.node(GAAST_OP_GEXP_ADJ2, g, h2, a2, 0x4, 3);
        gaast::Plan plan2;
        gaast::build_plan(k.desc(3, ones), plan2);
        CHECK(plan2.error == GAAST_ERR_INVALID_PROGRAM);
        for (int third : {-1, 3, 7}) {   // the third child must be an earlier node: build_plan throws, gaast_program_vjp says INVALID_PROGRAM
            Raw m;
            const int g3 = m.input(0x5, 3), h3 = m.input(0x4, 3);
            m.input(0x4, 3);
            m.node(GAAST_OP_GEXP_ADJ2, g3, h3, third, 0x4, 3);
            bool threw = false;
            try {
                gaast::Plan p3;
                gaast::build_plan(m.desc(3, ones), p3);
            } catch (const std::runtime_error&) {
                threw = true;
            }
            CHECK(threw);
            gaast_program_image_t img = nullptr;
            CHECK(gaast_program_vjp(&m.d, 0, &img) == GAAST_ERR_INVALID_PROGRAM && !img);
        }
        Raw big;   // N = 128: beyond the kernels
        const int hb = big.input(0x7, 7), ab = big.input(0x7, 7);
        big.node(GAAST_OP_GEXP_JVP, hb, ab, -1, 0xff, 7);
        gaast::Plan pb;
        gaast::build_plan(big.desc(7, ones), pb);
        CHECK(pb.error == GAAST_OK && !pb.unsupported.empty());
        std::printf("ok  raw malformed nodes\n");
    }
    for (gaast_expr_t h : handles) gaast_expr_release(h);
    if (failures) {
        std::printf("%d CHECKS FAILED\n", failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
