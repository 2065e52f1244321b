// Second order through the general logarithm on the host, under AddressSanitizer + UBSan (CPU build only; no GPU, no HIP, never loaded
// into Python): gaast_program_vjp with GAAST_FLAG_GSQRT_GLOG_JVP | GAAST_FLAG_GLOG_GRAD2, with either flag alone and with none, through
// {GLOG_ADJ, GLOG_JVP, GLOG_ADJ2} (host/vjp.cpp: root_log_family_adjoint) and the lowering into Step::GLOG_ADJ2 (plan.cpp:
// lower_glog_adj2) under every plan form, for n = 1 ... 7.  It also prints the tables of the lowered steps of hand-built programs
// ("GA2OUT ..." / "GA2TAB ..." lines) for tests/test_glog_adj2_host.py to compare with numpy.
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

static const uint32_t JVP = GAAST_FLAG_GSQRT_GLOG_JVP, GRAD2 = GAAST_FLAG_GLOG_GRAD2, BOTH = JVP | GRAD2;

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

// every table of a GLOG_ADJ2 step has its size, every offset stays inside the row it indexes, no result component is written twice, the
// four sign tables agree with each other, and all three operand rows are in the list of the step's reads
static void check_step(const gaast::Plan& plan, const gaast::Step& s) {
    const gaast::Layout &la = plan.layout(s.a), &lr = plan.layout(s.res);
    const gaast::Step::Inverse& q = s.inv;
    CHECK(s.a.idx >= 0 && s.b.idx >= 0 && s.c.idx >= 0);
    CHECK(!(s.a == s.res) && !(s.b == s.res) && !(s.c == s.res));
    CHECK(q.N == 2 || q.N == 4 || q.N == 8 || q.N == 16 || q.N == 32 || q.N == 64);
    CHECK(q.N == (1 << (q.even ? plan.n - 1 : plan.n)));
    const size_t N = size_t(q.N);
    CHECK(q.blade.size() == N && q.a_off.size() == N && q.res_off.size() == N && q.neg.size() == N && q.g_off.size() == N && q.h_off.size() == N);
    CHECK(q.rmul_neg.size() == N && q.adj_neg_l.size() == N && q.adj_neg_r.size() == N);
    CHECK(q.weight.size() == size_t(1) << plan.n && q.weight.size() <= 128);
    double wmax = 0;
    for (double w : q.weight) wmax = std::fmax(wmax, std::fabs(w));
    CHECK(q.wmax == wmax);
    if (q.g_off.size() != N || q.h_off.size() != N || q.rmul_neg.size() != N || q.adj_neg_l.size() != N || q.adj_neg_r.size() != N) return;
    std::vector<char> seen(size_t(lr.row_len), 0);
    int produced = 0;
    for (int j = 0; j < q.N; ++j) {
        CHECK(q.a_off[size_t(j)] >= -1 && int64_t(q.a_off[size_t(j)]) < la.row_len);
        CHECK(q.res_off[size_t(j)] >= -1 && int64_t(q.res_off[size_t(j)]) < lr.row_len);
        CHECK(q.g_off[size_t(j)] >= -1 && int64_t(q.g_off[size_t(j)]) < plan.layout(s.b).row_len);
        CHECK(q.h_off[size_t(j)] >= -1 && int64_t(q.h_off[size_t(j)]) < plan.layout(s.c).row_len);
        if (q.res_off[size_t(j)] >= 0) CHECK(q.a_off[size_t(j)] >= 0);   // the result lies within the operand's grades
        if (q.res_off[size_t(j)] >= 0 && int64_t(q.res_off[size_t(j)]) < lr.row_len) {
            CHECK(!seen[size_t(q.res_off[size_t(j)])]);
            seen[size_t(q.res_off[size_t(j)])] = 1;
            ++produced;
        }
        for (int r = 0; r < q.N; ++r) {
            CHECK(((q.rmul_neg[size_t(r)] >> j) & 1ULL) == ((q.neg[size_t(r)] >> (r ^ j)) & 1ULL));       // R[r][j]: the sign of L[r][r xor j]
            CHECK(((q.adj_neg_l[size_t(r)] >> j) & 1ULL) == ((q.neg[size_t(r ^ j)] >> j) & 1ULL));       // coeff(a = r, b = j): the sign of L[r xor j][j]
            CHECK(((q.adj_neg_r[size_t(j)] >> r) & 1ULL) == ((q.neg[size_t(r ^ j)] >> j) & 1ULL));
        }
    }
    CHECK(produced == q.n_out && produced > 0);
    if (s.beta == 0) CHECK(int64_t(produced) == lr.row_len);
    if (q.N < 64) CHECK((q.a_neg >> q.N) == 0);
    int hits = 0;
    gaast::for_each_read(s, [&](gaast::BufRef r) { hits += (r == s.a) + (r == s.b) + (r == s.c); });
    CHECK(hits >= 3);
    CHECK(s.name.rfind("general_log_adjoint2[", 0) == 0);
}

static void print_steps(const gaast::Plan& plan, const char* tag) {
    for (const gaast::Step& s : plan.steps) {
        if (s.kind != gaast::Step::GLOG_ADJ2) continue;
        const gaast::Step::Inverse& q = s.inv;
        for (int j = 0; j < q.N; ++j)
            std::printf("GA2OUT %s %d %d %u %d %d %d %d %d\n", tag, q.N, j, q.blade[size_t(j)], q.a_off[size_t(j)], q.res_off[size_t(j)],
                        q.g_off[size_t(j)], q.h_off[size_t(j)], int((q.a_neg >> j) & 1));
        for (int r = 0; r < q.N; ++r)
            for (int j = 0; j < q.N; ++j) {
                const double w = q.weight[size_t(q.blade[size_t(j)] & ~q.blade[size_t(r)])];   // of L[r][j] and of R[r][j]
                const double wa = q.weight[size_t(q.blade[size_t(r)] & q.blade[size_t(j)])];   // of coeff(r, j) and of coeff(j, r)
                std::printf("GA2TAB %s %d %d %.17g %.17g %.17g %.17g\n", tag, r, j, q.coeff(r, j), ((q.rmul_neg[size_t(r)] >> j) & 1ULL) ? -w : w,
                            ((q.adj_neg_l[size_t(r)] >> j) & 1ULL) ? -wa : wa, ((q.adj_neg_r[size_t(r)] >> j) & 1ULL) ? -wa : wa);
            }
    }
}

// lowers `d` under every plan form: as many GLOG_ADJ2 steps as nodes at the least, each a launch of its own
static void lower_all(const gaast_program_desc& d, const char* what, const char* tab = nullptr, bool supported = true) {
    const int n2 = count_op(d, GAAST_OP_GLOG_ADJ2);
    for (uint32_t extra : {0u, uint32_t(GAAST_FLAG_NO_FUSION), uint32_t(GAAST_FLAG_NO_JIT), uint32_t(GAAST_FLAG_EXACT_ORDER), uint32_t(GAAST_FLAG_DEBUG_JIT_FAILS)}) {
        gaast_program_desc b = d;
        b.flags |= extra;
        gaast::Plan plan;
        gaast::build_plan(b, plan);
        if (plan.error != GAAST_OK) std::printf("%s: plan error %d: %s\n", what, plan.error, plan.error_msg.c_str());
        CHECK(plan.error == GAAST_OK);
        if (!supported) {
            CHECK(!plan.unsupported.empty());
            continue;
        }
        if (!plan.unsupported.empty()) std::printf("%s: unsupported: %s\n", what, plan.unsupported.c_str());
        CHECK(plan.unsupported.empty());
        CHECK(count_steps(plan, gaast::Step::GLOG_ADJ2) >= n2 && (n2 > 0) == (count_steps(plan, gaast::Step::GLOG_ADJ2) > 0));
        CHECK(plan.has_glog == (count_steps(plan, gaast::Step::GLOG) > 0));
        CHECK(count_steps(plan, gaast::Step::FUSED) == 0 || n2 == 0);
        for (const gaast::Step& s : plan.steps)
            if (s.kind == gaast::Step::GLOG_ADJ2) check_step(plan, s);
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
    std::vector<unsigned char> again(gaast_program_serialize(&b, nullptr, 0));
    gaast_program_serialize(&b, again.data(), again.size());
    CHECK(again == buf);
    gaast_program_image_free(img);
}

// every GLOG_ADJ2 node of an image: three earlier children, the operand's mask
static void check_adj2_nodes(const gaast_program_desc& a) {
    for (int i = 0; i < a.n_nodes; ++i) {
        const gaast_node_desc& nd = a.nodes[i];
        if (nd.opcode != GAAST_OP_GLOG_ADJ2) continue;
        CHECK(nd.child0 >= 0 && nd.child0 < i && nd.child1 >= 0 && nd.child1 < i && nd.input_slot >= 0 && nd.input_slot < i);
        if (nd.input_slot >= 0 && nd.input_slot < i) CHECK(nd.minimal_grade_mask == a.nodes[nd.input_slot].minimal_grade_mask);
    }
}

static bool refused(const gaast_program_desc& a, int slot, const char* word) {
    gaast_program_image_t img = nullptr;
    const int st = gaast_program_vjp(&a, slot, &img);
    const bool ok = st == GAAST_ERR_UNIMPLEMENTED && !img && std::strstr(gaast_expr_last_error(), word) != nullptr;
    if (img) gaast_program_image_free(img);
    return ok;
}

// First order in every batched slot under the four flag settings.  Second order in every batched slot of each image: with both flags a
// slot under glog gives GLOG_ADJ2 nodes, which lower; with GAAST_FLAG_GSQRT_GLOG_JVP alone, and with GAAST_FLAG_GLOG_GRAD2 alone, the
// status and the words of today.  Third order through a GLOG_ADJ2 node is refused by name.
static void exercise(gaast_expr_t e, int n, const double* metric, const char* what, bool supported) {
    gaast_spec_t spec = gaast_expr_specialize(e, n, metric, 0);
    CHECK(spec != nullptr);
    if (!spec) return;
    int seen = 0, third = 0;
    for (int dtype : {GAAST_F64, GAAST_F32}) {
        gaast_program_desc d_jvp, d_g2, d_both;
        CHECK(gaast_spec_program_desc(spec, dtype, JVP, &d_jvp) == 0 && gaast_spec_program_desc(spec, dtype, GRAD2, &d_g2) == 0 &&
              gaast_spec_program_desc(spec, dtype, BOTH, &d_both) == 0);
        for (int s1 = 0; s1 < d_both.n_inputs; ++s1) {
            if (d_both.inputs[s1].is_const) continue;
            gaast_program_image_t i_jvp = nullptr, i_g2 = nullptr, i_both = nullptr;
            CHECK(gaast_program_vjp(&d_jvp, s1, &i_jvp) == 0 && gaast_program_vjp(&d_g2, s1, &i_g2) == 0 && gaast_program_vjp(&d_both, s1, &i_both) == 0);
            if (!i_jvp || !i_g2 || !i_both) continue;
            const gaast_program_desc &a_jvp = *gaast_program_image_desc(i_jvp), &a_g2 = *gaast_program_image_desc(i_g2), &a = *gaast_program_image_desc(i_both);
            CHECK(a.flags == (d_both.flags | BOTH) && count_op(a, GAAST_OP_GLOG_ADJ2) == 0 && count_op(a, GAAST_OP_GLOG_ADJ) > 0);
            CHECK(refused(a_jvp, s1, "GAAST_OP_GLOG_ADJ with respect to its operand"));
            CHECK(refused(a_g2, s1, "second-order reverse mode through GAAST_OP_GLOG_ADJ is not implemented"));
            gaast_program_image_t i2 = nullptr;
            CHECK(gaast_program_vjp(&a, s1, &i2) == 0 && i2);
            if (i2) {
                const gaast_program_desc& a2 = *gaast_program_image_desc(i2);
                CHECK(count_op(a2, GAAST_OP_GLOG_ADJ2) > 0);
                seen += count_op(a2, GAAST_OP_GLOG_ADJ2);
                check_adj2_nodes(a2);
                lower_all(a2, what, nullptr, supported);
                round_trip(a2);
                CHECK(refused(a2, s1, "third-order reverse mode through GAAST_OP_GLOG_ADJ2 is not implemented"));
                ++third;
                gaast_program_image_t j3 = nullptr;   // with respect to its first cotangent the second-order image holds the ADJ2 node off the path
                if (gaast_program_vjp(&a2, d_both.n_inputs, &j3) == 0 && j3) {
                    check_adj2_nodes(*gaast_program_image_desc(j3));
                    gaast_program_image_free(j3);
                }
                gaast_program_image_free(i2);
            }
            gaast_program_image_t j = nullptr;   // forward mode, then the tangent node's operand: GLOG_ADJ2(k, h, A)
            CHECK(gaast_program_vjp(&a, a.n_inputs - 1 - (a.inputs[a.n_inputs - 1].is_const ? 1 : 0), &j) == 0 && j);
            if (j) {
                const gaast_program_desc& aj = *gaast_program_image_desc(j);
                CHECK(count_op(aj, GAAST_OP_GLOG_JVP) > 0);
                gaast_program_image_t j2 = nullptr;
                CHECK(gaast_program_vjp(&aj, s1, &j2) == 0 && j2);
                if (j2) {
                    CHECK(count_op(*gaast_program_image_desc(j2), GAAST_OP_GLOG_ADJ2) > 0);
                    check_adj2_nodes(*gaast_program_image_desc(j2));
                    if (dtype == GAAST_F64) lower_all(*gaast_program_image_desc(j2), what, nullptr, supported);
                    gaast_program_image_free(j2);
                }
                gaast_program_image_free(j);
            }
            gaast_program_image_free(i_jvp);
            gaast_program_image_free(i_g2);
            gaast_program_image_free(i_both);
        }
    }
    CHECK(seen > 0 && third > 0);
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
    const double pga[4] = {0, 1, 1, 1}, cga[5] = {1, 1, 1, 1, -1}, odd[3] = {2, -0.5, 1}, ones[GAAST_MAX_DIM > 8 ? GAAST_MAX_DIM : 8] = {1, 1, 1, 1, 1, 1, 1, 1};
    for (int n = 1; n <= 7; ++n) {   // glog(x) over every blade (n <= 6) and over the even blades (n >= 2); n = 7 full: beyond the kernels
        const uint64_t full = (uint64_t(2) << n) - 1, even = full & 0x5555555555555555ULL;
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 1 && n == 1) continue;
            const std::string tag = std::string(pass ? "even" : "full") + " n=" + std::to_string(n);
            gaast_expr_t x = H(gaast_expr_input(0, pass ? even : full, n));
            exercise(H(gaast_expr_glog(x)), n, ones, ("glog(x) " + tag).c_str(), pass ? n <= 7 : n <= 6);
        }
    }
    {
        gaast_expr_t m = H(gaast_expr_input(0, 0x15, 4)), t = H(gaast_expr_input(1, 0x15, 4));
        gaast_expr_t pose = H(gaast_expr_glog(H(gaast_expr_product(m, H(gaast_expr_inv(t)), GAAST_PROD_GEOMETRIC))));
        exercise(pose, 4, pga, "glog(m * t.inv())", true);
        exercise(H(gaast_expr_g(pose, 2)), 4, pga, "glog(m * t.inv()).g(2)", true);
    }
    {   // the tables the host test compares with numpy: g and h hold parts of the blade set, the operand is read through a reverse
        Raw p;   // PGA3D: every blade; grade 2 and 3 negated in the read
        const int gp = p.input(0x17, 4), hp = p.input(0x0e, 4), bp = p.input(0x1f, 4);
        const int ap = p.node(GAAST_OP_REVERSE, bp, -1, -1, 0x1f, 4);
        p.node(GAAST_OP_GLOG_ADJ2, gp, hp, ap, 0x1f, 4);
        lower_all(p.desc(4, pga), "raw second-order adjoint, PGA3D", "pga");
        round_trip(p.d);
        Raw c;   // CGA: the even blades from a bivector operand, g a scalar and a 4-vector, h the bivectors
        const int gc = c.input(0x11, 5), hc = c.input(0x4, 5), ac = c.input(0x4, 5);
        c.node(GAAST_OP_GLOG_ADJ2, gc, hc, ac, 0x4, 5);
        lower_all(c.desc(5, cga), "raw second-order adjoint, CGA", "cga");
        round_trip(c.d);
        Raw o;   // a metric (2, -1/2, 1): the metric factors
        const int go = o.input(0xf, 3), ho = o.input(0xf, 3), ao = o.input(0xf, 3);
        o.node(GAAST_OP_GLOG_ADJ2, go, ho, ao, 0xf, 3);
        lower_all(o.desc(3, odd), "raw second-order adjoint, metric (2, -1/2, 1)", "odd");
        std::printf("ok  raw tables\n");
    }
    {   // malformed nodes of the raw ABI are refused, not read out of bounds
        for (int which = 0; which < 2; ++which) {   // g, then h, with a grade outside the blade set
            Raw j;
            const int g = j.input(which == 0 ? 0x2 : 0x5, 3), h = j.input(which == 1 ? 0x2 : 0x5, 3), a = j.input(0x4, 3);
            j.node(GAAST_OP_GLOG_ADJ2, g, h, a, 0x4, 3);
            gaast::Plan plan;
            gaast::build_plan(j.desc(3, ones), plan);
            CHECK(plan.error == GAAST_ERR_INVALID_PROGRAM);
        }
        for (int third : {-1, 3, 9}) {   // the operand must be an earlier node
            Raw m;
            const int g = m.input(0x5, 3), h = m.input(0x5, 3);
            m.input(0x5, 3);
            m.node(GAAST_OP_GLOG_ADJ2, g, h, third, 0x5, 3);
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
        const int gb = big.input(0x7, 7), hb = big.input(0x7, 7), ab = big.input(0x7, 7);
        big.node(GAAST_OP_GLOG_ADJ2, gb, hb, ab, 0x7, 7);
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
