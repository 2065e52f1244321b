// Complements and the regressive product on the host, under AddressSanitizer + UBSan (CPU build only; no GPU, no HIP, never
// loaded into Python): list generation and its closed-form count (common/comp_mul_table.hpp), grade inference and the phase-3
// restriction (host/expr.cpp), the wire format, gaast_program_vjp through GAAST_OP_DUAL / GAAST_OP_UNDUAL and
// GAAST_PROD_REGRESSIVE (host/vjp.cpp), the lowering into Step::DUAL and regressive lists (plan.cpp: lower_dual, lower_product)
// with and without the orientation sign of a Gram basis, and the statements generated for gaast_jit (plan_fused.cpp).
// It also prints the sign tables of Step::DUAL ("DUALTAB ..." lines) for tests/test_dual_host.py to compare with numpy.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gaast_expr.h"
#include "metric_basis.hpp"
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

// every offset of a DUAL step stays inside the rows it indexes, and no result component is written twice
static void check_dual_step(const gaast::Plan& plan, const gaast::Step& s) {
    const gaast::Layout &la = plan.layout(s.a), &lr = plan.layout(s.res);
    CHECK(!(s.a == s.res));
    CHECK(s.dual.total > 0 && s.dual.neg.size() == size_t((s.dual.total + 31) / 32));
    CHECK(s.dual.segs.size() <= size_t(GAAST_MAX_DIM + 1));
    std::vector<char> seen(size_t(lr.row_len), 0);
    int count = 0;
    s.dual.for_each([&](uint32_t r, uint32_t a, bool) {
        CHECK(int64_t(a) < la.row_len && int64_t(r) < lr.row_len);
        if (int64_t(r) < lr.row_len) {
            CHECK(!seen[r]);
            seen[r] = 1;
        }
        ++count;
    });
    CHECK(count == s.dual.total);
    if (s.beta == 0) CHECK(int64_t(count) == lr.row_len);
}

static void print_dual_steps(const gaast::Plan& plan, const char* tag) {
    for (const gaast::Step& s : plan.steps)
        if (s.kind == gaast::Step::DUAL)
            s.dual.for_each([&](uint32_t r, uint32_t a, bool neg) { std::printf("DUALTAB %s %d %d %u %u %d\n", tag, plan.n, s.dual.undual, r, a, neg ? 1 : 0); });
}

static int count_op(const gaast_program_desc& d, int opcode) {
    int c = 0;
    for (int i = 0; i < d.n_nodes; ++i) c += d.nodes[i].opcode == opcode;
    return c;
}

// lowers `d` under every plan form; returns the number of launches of the default plan
static size_t lower_all(const gaast_program_desc& d, const char* what) {
    size_t default_steps = 0;
    for (int mirrored = 0; mirrored < 2; ++mirrored)
        for (uint32_t extra : {0u, uint32_t(GAAST_FLAG_NO_FUSION), uint32_t(GAAST_FLAG_NO_JIT), uint32_t(GAAST_FLAG_EXACT_ORDER)}) {
            gaast_program_desc b = d;
            b.flags |= extra;
            gaast::Plan plan;
            gaast::build_plan(b, plan, false, mirrored != 0);
            if (plan.error != GAAST_OK) std::printf("%s: plan error %d: %s\n", what, plan.error, plan.error_msg.c_str());
            CHECK(plan.error == GAAST_OK && plan.unsupported.empty());
            CHECK(plan.mirrored == mirrored);
            for (const gaast::Step& s : plan.steps) {
                if (s.kind == gaast::Step::DUAL) check_dual_step(plan, s);
            }
            if (!mirrored && !extra) default_steps = plan.steps.size();
        }
    return default_steps;
}

static void round_trip(const gaast_program_desc& a) {
    const size_t need = gaast_program_serialize(&a, nullptr, 0);
    std::vector<unsigned char> buf(need);
    CHECK(gaast_program_serialize(&a, buf.data(), need) == need);
    gaast_program_image_t img = gaast_program_deserialize(buf.data(), need);
    CHECK(img != nullptr);
    if (img) {
        const gaast_program_desc& b = *gaast_program_image_desc(img);
        CHECK(b.n_nodes == a.n_nodes && b.root == a.root);
        for (int i = 0; i < a.n_nodes && i < b.n_nodes; ++i) {
            CHECK(a.nodes[i].opcode == b.nodes[i].opcode && a.nodes[i].product_kind == b.nodes[i].product_kind);
            CHECK(a.nodes[i].n_comp_muls == b.nodes[i].n_comp_muls && (a.nodes[i].comp_muls != nullptr) == (b.nodes[i].comp_muls != nullptr));
            if (a.nodes[i].comp_muls && b.nodes[i].comp_muls)
                CHECK(std::memcmp(a.nodes[i].comp_muls, b.nodes[i].comp_muls, size_t(a.nodes[i].n_comp_muls) * sizeof(gaast_comp_mul)) == 0);
        }
        gaast_program_image_free(img);
    }
    for (size_t cut = 0; cut < need; cut += need / 5 + 1) CHECK(gaast_program_deserialize(buf.data(), cut) == nullptr);
}

// specialise (explicit lists, or compact with limit 1), lower, serialise, differentiate with respect to every batched slot
// tab: the program is dual(x) / undual(x) of one input; its sign tables are printed
static size_t exercise(gaast_expr_t e, int n, const double* metric, const char* what, const char* tab = nullptr) {
    size_t launches = 0;
    for (uint64_t limit : {uint64_t(0), uint64_t(1)}) {
        gaast_spec_t spec = gaast_expr_specialize(e, n, metric, limit);
        if (!spec) std::printf("%s: %s\n", what, gaast_expr_last_error());
        CHECK(spec != nullptr);
        if (!spec) return 0;
        for (int i = 0; i < gaast_spec_num_nodes(spec); ++i) {   // the closed-form count is the list's length
            gaast_spec_node_info info;
            CHECK(gaast_spec_node(spec, i, &info) == 0);
            if (info.opcode == GAAST_OP_PRODUCT && limit == 0) CHECK(gaast_spec_comp_muls(spec, i) != nullptr || info.n_comp_muls == 0);
        }
        for (int dtype : {GAAST_F64, GAAST_F32}) {
            gaast_program_desc desc;
            CHECK(gaast_spec_program_desc(spec, dtype, 0, &desc) == 0);
            const size_t steps = lower_all(desc, what);
            if (limit == 0 && dtype == GAAST_F64) launches = steps;
            round_trip(desc);
            if (tab && limit == 0 && dtype == GAAST_F64)
                for (int mirrored = 0; mirrored < 2; ++mirrored) {
                    gaast_program_desc b = desc;
                    b.flags |= GAAST_FLAG_NO_FUSION;
                    gaast::Plan plan;
                    gaast::build_plan(b, plan, false, mirrored != 0);
                    print_dual_steps(plan, (std::string(tab) + (mirrored ? "-mirrored" : "")).c_str());
                }
            for (int slot = 0; slot < desc.n_inputs; ++slot) {
                if (desc.inputs[slot].is_const) continue;
                gaast_program_image_t img = nullptr;
                const int st = gaast_program_vjp(&desc, slot, &img);
                if (st) std::printf("%s: vjp status %d: %s\n", what, st, gaast_expr_last_error());
                CHECK(st == 0 && img != nullptr);
                if (!img) continue;
                const gaast_program_desc& a = *gaast_program_image_desc(img);
                if (tab)   // dual(x) / undual(x): the transpose of a complement is the other complement, of the cotangent
                    CHECK(count_op(a, GAAST_OP_DUAL) == (std::strcmp(tab, "undual") == 0) && count_op(a, GAAST_OP_UNDUAL) == (std::strcmp(tab, "dual") == 0));
                lower_all(a, what);
                round_trip(a);
                gaast_program_image_free(img);
            }
        }
        gaast_spec_free(spec);
    }
    std::printf("ok  %s (%zu launches)\n", what, launches);
    return launches;
}

int main() {
    const double pga[4] = {0, 1, 1, 1}, cga[5] = {1, 1, 1, 1, -1};
    double ones[GAAST_MAX_DIM];
    for (double& v : ones) v = 1.0;
    // complements of a full multivector, n = 1 .. 8: the sign tables
    for (int n = 1; n <= 8; ++n) {
        const uint64_t full = (uint64_t(1) << (n + 1)) - 1;
        exercise(H(gaast_expr_dual(H(gaast_expr_input(0, full, n)))), n, ones, "dual(x)", "dual");
        exercise(H(gaast_expr_undual(H(gaast_expr_input(0, full, n)))), n, ones, "undual(x)", "undual");
    }
    {   // an interior operand, a sign-only chain over an input folded into the signs, a scalar literal, undual(dual(x)) + x
        gaast_expr_t a = H(gaast_expr_input(0, 1u << 1, 4)), b = H(gaast_expr_input(1, 1u << 2, 4));
        exercise(H(gaast_expr_dual(H(gaast_expr_product(a, b, GAAST_PROD_OUTER)))), 4, pga, "dual(a ^ b)");
        exercise(H(gaast_expr_dual(H(gaast_expr_rev(b)))), 4, pga, "dual(~b)");
        exercise(H(gaast_expr_dual(H(gaast_expr_from_f64(2.5)))), 4, pga, "dual(2.5)");   // a scalar literal (storage dimension 0) -> grade n
        gaast_expr_t x = H(gaast_expr_input(0, 0x1f, 4));
        exercise(H(gaast_expr_add(H(gaast_expr_undual(H(gaast_expr_dual(x)))), x)), 4, pga, "undual(dual(x)) + x");
        exercise(H(gaast_expr_g(H(gaast_expr_dual(x)), 3)), 4, pga, "dual(x).g(3)");
    }
    {   // PGA3D: join of three points (grade-3 trivectors) and meet of two planes (vectors): one launch each
        gaast_expr_t p1 = H(gaast_expr_input(0, 1u << 3, 4)), p2 = H(gaast_expr_input(1, 1u << 3, 4)), p3 = H(gaast_expr_input(2, 1u << 3, 4));
        gaast_expr_t join = H(gaast_expr_product(H(gaast_expr_product(p1, p2, GAAST_PROD_REGRESSIVE)), p3, GAAST_PROD_REGRESSIVE));
        CHECK(exercise(join, 4, pga, "PGA3D p1 v p2 v p3") == 1);
        gaast_expr_t pl1 = H(gaast_expr_input(0, 1u << 1, 4)), pl2 = H(gaast_expr_input(1, 1u << 1, 4));
        // grade 1 + 1 - 4 < 0: an empty program, not an error
        exercise(H(gaast_expr_product(pl1, pl2, GAAST_PROD_REGRESSIVE)), 4, pga, "vector v vector (empty)");
        gaast_expr_t t1 = H(gaast_expr_input(0, 1u << 3, 4)), b2 = H(gaast_expr_input(1, 1u << 2, 4));
        exercise(H(gaast_expr_product(t1, b2, GAAST_PROD_REGRESSIVE)), 4, pga, "trivector v bivector");
    }
    {   // full multivectors, the restriction (a v b).g(1), CGA
        for (int n = 2; n <= 6; ++n) {
            const uint64_t full = (uint64_t(1) << (n + 1)) - 1;
            gaast_expr_t a = H(gaast_expr_input(0, full, n)), b = H(gaast_expr_input(1, full, n));
            gaast_expr_t v = H(gaast_expr_product(a, b, GAAST_PROD_REGRESSIVE));
            exercise(v, n, ones, "a v b full");
            exercise(H(gaast_expr_g(v, 1)), n, ones, "(a v b).g(1)");
        }
        gaast_expr_t s1 = H(gaast_expr_input(0, 1u << 4, 5)), s2 = H(gaast_expr_input(1, 1u << 4, 5));
        exercise(H(gaast_expr_product(s1, s2, GAAST_PROD_REGRESSIVE)), 5, cga, "CGA meet of two spheres");
    }
    {   // the regressive list as it is lowered, with and without the orientation sign ("VEETAB ..." lines); explicit and compact
        gaast_expr_t a = H(gaast_expr_input(0, 0xf, 3)), b = H(gaast_expr_input(1, 0xf, 3));
        gaast_expr_t v = H(gaast_expr_product(a, b, GAAST_PROD_REGRESSIVE));
        for (uint64_t limit : {uint64_t(0), uint64_t(1)}) {
            gaast_spec_t spec = gaast_expr_specialize(v, 3, ones, limit);
            CHECK(spec != nullptr);
            if (!spec) continue;
            gaast_program_desc desc;
            CHECK(gaast_spec_program_desc(spec, GAAST_F64, GAAST_FLAG_NO_FUSION, &desc) == 0);
            for (int mirrored = 0; mirrored < 2; ++mirrored) {
                gaast::Plan plan;
                gaast::build_plan(desc, plan, false, mirrored != 0);
                for (const gaast::Step& s : plan.steps)
                    if (s.kind == gaast::Step::PRODUCT_CSR)
                        for (size_t row = 0; row + 1 < s.list.row_start.size(); ++row)
                            for (uint32_t e = s.list.row_start[row]; e < s.list.row_start[row + 1]; ++e)
                                std::printf("VEETAB %s%s %u %u %u %g\n", limit ? "compact" : "explicit", mirrored ? "-mirrored" : "", s.list.row_out[row],
                                            s.list.entries[e] & 0xffffu, s.list.entries[e] >> 16, s.list.coeff[e]);
            }
            gaast_spec_free(spec);
        }
    }
    {   // a plan with complements is ONE fused launch as the specialised kernel, and as the interpreter's micro-ops without it
        gaast_expr_t a = H(gaast_expr_input(0, 1u << 3, 4)), b = H(gaast_expr_input(1, 1u << 3, 4));
        gaast_expr_t e = H(gaast_expr_undual(H(gaast_expr_product(H(gaast_expr_dual(a)), H(gaast_expr_dual(b)), GAAST_PROD_OUTER))));
        gaast_spec_t spec = gaast_expr_specialize(e, 4, pga, 0);
        CHECK(spec != nullptr);
        for (uint32_t flags : {0u, uint32_t(GAAST_FLAG_NO_JIT)}) {
            gaast_program_desc desc;
            CHECK(gaast_spec_program_desc(spec, GAAST_F32, flags, &desc) == 0);
            gaast::Plan plan;
            gaast::build_plan(desc, plan);
            CHECK(plan.steps.size() == 1 && plan.steps[0].kind == gaast::Step::FUSED);
            if (plan.steps.size() == 1) {
                CHECK(plan.steps[0].fused.jit_source.empty() == (flags != 0) && plan.steps[0].fused.jit_only == 0);
                CHECK(!plan.steps[0].fused.prog.empty());
            }
        }
        gaast_spec_free(spec);
        // a run of element-wise arms absorbs a complement of a bound input: x + dual(y) at n = 9 is one pass
        const uint64_t full = (uint64_t(1) << 10) - 1;
        gaast_expr_t x = H(gaast_expr_input(0, full, 9)), y = H(gaast_expr_input(1, full, 9));
        spec = gaast_expr_specialize(H(gaast_expr_add(x, H(gaast_expr_dual(y)))), 9, ones, 0);
        CHECK(spec != nullptr);
        gaast_program_desc desc;
        CHECK(gaast_spec_program_desc(spec, GAAST_F64, 0, &desc) == 0);
        gaast::Plan plan;
        gaast::build_plan(desc, plan);
        CHECK(plan.steps.size() == 1 && plan.steps[0].kind == gaast::Step::ELEMENTWISE && plan.steps[0].ew.src.size() == 2);
        gaast_spec_free(spec);
        std::printf("ok  fused forms of complement plans\n");
    }
    {   // the orientation of a Gram basis, from a constructed Q: a rotation (det +1) and the same with two columns swapped (det -1)
        const double c = 0.6, s = 0.8;
        const double rot[9] = {c, -s, 0, s, c, 0, 0, 0, 1}, swapped[9] = {-s, c, 0, c, s, 0, 0, 0, 1};
        CHECK(std::fabs(gaast::matrix_determinant(3, rot) - 1.0) < 1e-15 && !gaast::basis_is_mirrored(3, rot));
        CHECK(std::fabs(gaast::matrix_determinant(3, swapped) + 1.0) < 1e-15 && gaast::basis_is_mirrored(3, swapped));
        const double eye[4] = {1, 0, 0, 1}, refl[4] = {0, 1, 1, 0};
        CHECK(!gaast::basis_is_mirrored(2, eye) && gaast::basis_is_mirrored(2, refl));
        // ... and through the lowering: the sign of dual(x) flips with it
        gaast_spec_t spec = gaast_expr_specialize(H(gaast_expr_dual(H(gaast_expr_input(0, 0xf, 3)))), 3, ones, 0);
        CHECK(spec != nullptr);
        gaast_program_desc desc;
        CHECK(gaast_spec_program_desc(spec, GAAST_F64, GAAST_FLAG_NO_FUSION, &desc) == 0);
        std::vector<int> signs[2];
        for (int m = 0; m < 2; ++m) {
            gaast::Plan plan;
            gaast::build_plan(desc, plan, false, gaast::basis_is_mirrored(3, m ? swapped : rot));
            for (const gaast::Step& st : plan.steps)
                if (st.kind == gaast::Step::DUAL) st.dual.for_each([&](uint32_t, uint32_t, bool neg) { signs[m].push_back(neg); });
        }
        CHECK(signs[0].size() == 8 && signs[1].size() == 8);
        for (size_t i = 0; i < signs[0].size() && i < signs[1].size(); ++i) CHECK(signs[0][i] != signs[1][i]);
        gaast_spec_free(spec);
        std::printf("ok  det Q from a constructed basis\n");
    }
    CHECK(gaast_expr_product(handles[0], handles[0], GAAST_PROD_REGRESSIVE + 1) == nullptr);
    for (gaast_expr_t h : handles) gaast_expr_release(h);
    if (failures) {
        std::printf("%d CHECKS FAILED\n", failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
