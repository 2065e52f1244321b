// Reverse mode through exp / log on the host, under AddressSanitizer + UBSan (CPU build only; no GPU, no HIP, never loaded
// into Python): gaast_program_vjp with GAAST_FLAG_EXP_LOG | GAAST_FLAG_EXP_LOG_GRAD (host/vjp.cpp: explog_adjoint), the
// lowering of GAAST_OP_EXP_ADJ / GAAST_OP_LOG_ADJ (plan.cpp: lower_exp_log_adj) into Step::EXPLOG_ADJ, the statements
// generated for gaast_jit (plan_fused.cpp: explog_adj_statements), the wire format, and the refusals.
#include <cstdio>
#include <cstring>
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

static const uint32_t GRAD = GAAST_FLAG_EXP_LOG | GAAST_FLAG_EXP_LOG_GRAD;

static int count_op(const gaast_program_desc& d, int opcode) {
    int c = 0;
    for (int i = 0; i < d.n_nodes; ++i) c += d.nodes[i].opcode == opcode;
    return c;
}

// every table and offset of an EXPLOG_ADJ step stays inside the rows it indexes
static void check_adj_step(const gaast::Plan& plan, const gaast::Step& s) {
    const gaast::Step::ExpLogAdj& q = s.adj;
    const gaast::Layout &la = plan.layout(s.a), &lg = plan.layout(s.b), &lr = plan.layout(s.res);
    CHECK(int(q.sq.size()) == q.m && q.m > 0);
    CHECK(q.arg_k >= 0 && q.arg_k + q.m <= la.row_len);
    CHECK(q.arg_0 < la.row_len);
    CHECK(q.mg <= q.m && (q.g_k >= 0 ? q.g_k + q.mg <= lg.row_len : q.mg == 0));
    CHECK(q.g_0 < lg.row_len);
    CHECK(q.mres <= q.m && (q.res_k >= 0 ? q.res_k + q.mres <= lr.row_len : q.mres == 0));
    CHECK(q.res_0 < lr.row_len);
    CHECK(!(s.a == s.res) && !(s.b == s.res));
    for (double v : q.sq) CHECK(v == v);
}

// VJP of `e` with respect to slot `wrt`, lowered under every plan the adjoint kernel or statements run in
static void vjp_and_lower(gaast_expr_t e, int n, const double* metric, int wrt, int adj_opcode, int want_adj, const char* what) {
    gaast_spec_t spec = gaast_expr_specialize(e, n, metric, 1 << 16);
    CHECK(spec != nullptr);
    if (!spec) return;
    for (int dtype : {GAAST_F64, GAAST_F32}) {
        gaast_program_desc desc;
        CHECK(gaast_spec_program_desc(spec, dtype, GRAD, &desc) == 0);
        gaast_program_image_t img = nullptr;
        const int st = gaast_program_vjp(&desc, wrt, &img);
        if (st) std::printf("%s: vjp status %d: %s\n", what, st, gaast_expr_last_error());
        CHECK(st == 0 && img != nullptr);
        if (!img) continue;
        const gaast_program_desc& a = *gaast_program_image_desc(img);
        CHECK(count_op(a, adj_opcode) == want_adj);
        CHECK(a.flags == desc.flags);
        for (int i = 0; i < a.n_nodes; ++i)
            if (a.nodes[i].opcode == GAAST_OP_EXP_ADJ || a.nodes[i].opcode == GAAST_OP_LOG_ADJ) {
                const gaast_node_desc& nd = a.nodes[i];
                CHECK(nd.child0 >= 0 && nd.child0 < i && nd.child1 >= 0 && nd.child1 < i);
                CHECK(nd.minimal_grade_mask == a.nodes[nd.child1].minimal_grade_mask);
            }
        for (uint32_t extra : {0u, uint32_t(GAAST_FLAG_NO_FUSION), uint32_t(GAAST_FLAG_NO_JIT), uint32_t(GAAST_FLAG_EXACT_ORDER)}) {
            gaast_program_desc b = a;
            b.flags |= extra;
            gaast::Plan plan;
            gaast::build_plan(b, plan);
            CHECK(plan.error == GAAST_OK && plan.unsupported.empty());
            CHECK(plan.has_explog_adj == (want_adj > 0 ? 1 : 0));
            if (!want_adj) continue;
            int adj_steps = 0, jit_adj = 0;
            for (const gaast::Step& s : plan.steps) {
                if (s.kind == gaast::Step::EXPLOG_ADJ) {
                    ++adj_steps;
                    check_adj_step(plan, s);
                }
                if (s.kind == gaast::Step::FUSED) {
                    CHECK(!s.fused.jit_source.empty() && s.fused.jit_only == 1);   // no interpreter form of the adjoint
                    jit_adj += s.fused.jit_source.find("dd = dd + ") != std::string::npos || s.fused.jit_source.find(" * w);") != std::string::npos;
                }
            }
            const int all_adj = count_op(a, GAAST_OP_EXP_ADJ) + count_op(a, GAAST_OP_LOG_ADJ);
            if (extra & (GAAST_FLAG_NO_FUSION | GAAST_FLAG_NO_JIT)) CHECK(adj_steps == all_adj && jit_adj == 0);
            else CHECK(adj_steps == 0 && jit_adj == 1 && plan.steps.size() == 1);
        }
        // the wire format carries the opcodes
        const size_t need = gaast_program_serialize(&a, nullptr, 0);
        std::vector<unsigned char> buf(need);
        CHECK(gaast_program_serialize(&a, buf.data(), need) == need);
        gaast_program_image_t img2 = gaast_program_deserialize(buf.data(), need);
        CHECK(img2 != nullptr);
        if (img2) {
            CHECK(count_op(*gaast_program_image_desc(img2), adj_opcode) == want_adj);
            gaast_program_image_free(img2);
        }
        for (size_t cut = 0; cut < need; cut += need / 5 + 1) CHECK(gaast_program_deserialize(buf.data(), cut) == nullptr);
        gaast_program_image_free(img);
    }
    gaast_spec_free(spec);
    std::printf("ok  %s\n", what);
}

int main() {
    const double r3[3] = {1, 1, 1}, pga[4] = {0, 1, 1, 1}, cga[5] = {1, 1, 1, 1, -1}, r21[3] = {1, 1, -1};
    {   // x.exp() * y
        gaast_expr_t x = H(gaast_expr_input(0, 1u << 2, 3)), y = H(gaast_expr_input(1, 1u << 2, 3));
        gaast_expr_t e = H(gaast_expr_product(H(gaast_expr_exp(x)), y, GAAST_PROD_GEOMETRIC));
        vjp_and_lower(e, 3, r3, 0, GAAST_OP_EXP_ADJ, 1, "exp(x) * y wrt x");
        // EXP_LOG alone: no adjoint through exp, the status of before
        gaast_spec_t spec = gaast_expr_specialize(e, 3, r3, 1 << 16);
        gaast_program_desc desc;
        CHECK(gaast_spec_program_desc(spec, GAAST_F64, GAAST_FLAG_EXP_LOG, &desc) == 0);
        gaast_program_image_t img = nullptr;
        CHECK(gaast_program_vjp(&desc, 0, &img) == GAAST_ERR_UNIMPLEMENTED && img == nullptr);
        CHECK(gaast_program_vjp(&desc, 1, &img) == 0 && img != nullptr);
        if (img) {
            CHECK(count_op(*gaast_program_image_desc(img), GAAST_OP_EXP_ADJ) == 0);
            gaast_program_image_free(img);
        }
        // an adjoint program whose flags lost GAAST_FLAG_EXP_LOG is refused whole
        CHECK(gaast_spec_program_desc(spec, GAAST_F64, GRAD, &desc) == 0);
        CHECK(gaast_program_vjp(&desc, 0, &img) == 0);
        if (img) {
            gaast_program_desc b = *gaast_program_image_desc(img);
            b.flags &= ~uint32_t(GAAST_FLAG_EXP_LOG);
            gaast::Plan plan;
            gaast::build_plan(b, plan);
            CHECK(!plan.unsupported.empty());
            gaast_program_image_free(img);
        }
        gaast_spec_free(spec);
    }
    {   // the motor sandwich exp(B) X ~exp(B) in PGA3D, with respect to both
        gaast_expr_t b = H(gaast_expr_input(0, 1u << 2, 4)), x = H(gaast_expr_input(1, 1u << 3, 4));
        gaast_expr_t r = H(gaast_expr_exp(b));
        gaast_expr_t e = H(gaast_expr_product(H(gaast_expr_product(r, x, GAAST_PROD_GEOMETRIC)), H(gaast_expr_rev(r)), GAAST_PROD_GEOMETRIC));
        vjp_and_lower(e, 4, pga, 0, GAAST_OP_EXP_ADJ, 2, "PGA3D exp(B) X ~exp(B) wrt B");
        vjp_and_lower(e, 4, pga, 1, GAAST_OP_EXP_ADJ, 0, "PGA3D exp(B) X ~exp(B) wrt X (no adjoint node)");
    }
    {   // log of a CGA versor with and without grade 0, log(exp(B)), vectors in R^{2,1}
        vjp_and_lower(H(gaast_expr_log(H(gaast_expr_input(0, 1u | (1u << 2), 5)))), 5, cga, 0, GAAST_OP_LOG_ADJ, 1, "CGA log(a + B)");
        vjp_and_lower(H(gaast_expr_log(H(gaast_expr_exp(H(gaast_expr_input(0, 1u << 2, 3)))))), 3, r3, 0, GAAST_OP_LOG_ADJ, 1, "log(exp(B))");
        vjp_and_lower(H(gaast_expr_exp(H(gaast_expr_input(0, 1u << 1, 3)))), 3, r21, 0, GAAST_OP_EXP_ADJ, 1, "exp(v), R^{2,1}");
    }
    {   // log of a bare bivector (phases 1-3 refuse it like the reference; the raw ABI does not): no grade 0 in the operand, no da
        gaast_node_desc nodes[2];
        std::memset(nodes, 0, sizeof(nodes));
        for (gaast_node_desc& nd : nodes) {
            nd.child0 = nd.child1 = nd.input_slot = -1;
            nd.vec_space_dim = 5;
            nd.minimal_grade_mask = 1u << 2;
            nd.product_kind = GAAST_PROD_EXPLICIT;
        }
        nodes[0].opcode = GAAST_OP_INPUT;
        nodes[0].input_slot = 0;
        nodes[1].opcode = GAAST_OP_LOG;
        nodes[1].child0 = 0;
        gaast_input_desc in{1u << 2, 5, 0, nullptr};
        gaast_program_desc d{5, cga, GAAST_F32, 2, nodes, 1, 1, &in, GRAD | GAAST_FLAG_NO_FUSION};
        gaast_program_image_t img = nullptr;
        CHECK(gaast_program_vjp(&d, 0, &img) == 0 && img != nullptr);
        if (img) {
            gaast::Plan plan;
            gaast::build_plan(*gaast_program_image_desc(img), plan);
            int seen = 0;
            for (const gaast::Step& s : plan.steps)
                if (s.kind == gaast::Step::EXPLOG_ADJ) {
                    check_adj_step(plan, s);
                    CHECK(s.adj.op == 1 && s.adj.arg_0 < 0 && s.adj.res_0 < 0 && s.adj.m == 10);
                    ++seen;
                }
            CHECK(seen == 1);
            gaast_program_image_free(img);
        }
        std::printf("ok  CGA log(B), raw ABI\n");
    }
    {   // exp of a bare scalar through the raw ABI: no adjoint node, a clear status
        gaast_node_desc nodes[2];
        std::memset(nodes, 0, sizeof(nodes));
        for (gaast_node_desc& nd : nodes) {
            nd.child0 = nd.child1 = nd.input_slot = -1;
            nd.vec_space_dim = 3;
            nd.minimal_grade_mask = 1;
            nd.product_kind = GAAST_PROD_EXPLICIT;
        }
        nodes[0].opcode = GAAST_OP_INPUT;
        nodes[0].input_slot = 0;
        nodes[1].opcode = GAAST_OP_EXP;
        nodes[1].child0 = 0;
        gaast_input_desc in{1, 3, 0, nullptr};
        gaast_program_desc d{3, r3, GAAST_F64, 2, nodes, 1, 1, &in, GRAD};
        gaast_program_image_t img = nullptr;
        CHECK(gaast_program_vjp(&d, 0, &img) == GAAST_ERR_UNIMPLEMENTED && img == nullptr);
        CHECK(std::strstr(gaast_expr_last_error(), "bare scalar") != nullptr);
    }
    for (gaast_expr_t h : handles) gaast_expr_release(h);
    if (failures) {
        std::printf("%d CHECKS FAILED\n", failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
