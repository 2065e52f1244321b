// The general multivector inverse on the host, under AddressSanitizer + UBSan (CPU build only; no GPU, no HIP, never loaded into
// Python): grade inference and the phase-3 restriction (host/expr.cpp), the wire format, gaast_program_vjp through GAAST_OP_INV
// (host/vjp.cpp) and the lowering into Step::INVERSE (plan.cpp: lower_inverse) for n = 1 ... 7 (8 for the refusal), full and even
// operands, under every plan form.
// It also prints the matrix of a lowered Step::INVERSE ("INVTAB ..." / "INVOUT ..." lines) for tests/test_inverse_host.py to
// compare with numpy, and the opcode census of the VJP programs ("VJPOPS ..." lines).
#include <cmath>
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

// every table of an INVERSE step has its size, every offset stays inside the row it indexes, no result component is written twice
static void check_inverse_step(const gaast::Plan& plan, const gaast::Step& s) {
    const gaast::Layout &la = plan.layout(s.a), &lr = plan.layout(s.res);
    const gaast::Step::Inverse& q = s.inv;
    CHECK(!(s.a == s.res));
    CHECK(q.N == 2 || q.N == 4 || q.N == 8 || q.N == 16 || q.N == 32 || q.N == 64);
    CHECK(q.N == (1 << (q.even ? plan.n - 1 : plan.n)));
    CHECK(q.blade.size() == size_t(q.N) && q.a_off.size() == size_t(q.N) && q.res_off.size() == size_t(q.N) && q.neg.size() == size_t(q.N));
    CHECK(q.weight.size() == size_t(1) << plan.n);
    std::vector<char> seen(size_t(lr.row_len), 0);
    int produced = 0;
    for (int j = 0; j < q.N && size_t(j) < q.blade.size(); ++j) {
        CHECK(q.blade[size_t(j)] < (1u << plan.n));
        if (j) CHECK(q.blade[size_t(j)] > q.blade[size_t(j - 1)]);
        CHECK(q.a_off[size_t(j)] >= -1 && int64_t(q.a_off[size_t(j)]) < la.row_len);
        CHECK(q.res_off[size_t(j)] >= -1 && int64_t(q.res_off[size_t(j)]) < lr.row_len);
        if (q.res_off[size_t(j)] >= 0 && int64_t(q.res_off[size_t(j)]) < lr.row_len) {
            CHECK(!seen[size_t(q.res_off[size_t(j)])]);
            seen[size_t(q.res_off[size_t(j)])] = 1;
            ++produced;
        }
        for (int r = 0; r < q.N; ++r) {   // the index rule the kernel relies on, and the table the metric factor is read from
            uint32_t x = q.blade[size_t(r)] ^ q.blade[size_t(j)];
            CHECK((q.even ? x >> 1 : x) == uint32_t(r ^ j));
            CHECK((q.blade[size_t(j)] & ~q.blade[size_t(r)]) < q.weight.size());
        }
    }
    CHECK(produced == q.n_out && produced > 0);
    if (s.beta == 0) CHECK(int64_t(produced) == lr.row_len);
    if (q.N < 64) CHECK((q.a_neg >> q.N) == 0);
}

static void print_inverse_steps(const gaast::Plan& plan, const char* tag) {
    for (const gaast::Step& s : plan.steps) {
        if (s.kind != gaast::Step::INVERSE) continue;
        const gaast::Step::Inverse& q = s.inv;
        for (int j = 0; j < q.N; ++j) std::printf("INVOUT %s %d %d %u %d %d %d\n", tag, q.N, j, q.blade[size_t(j)], q.a_off[size_t(j)], q.res_off[size_t(j)], int((q.a_neg >> j) & 1));
        for (int r = 0; r < q.N; ++r)
            for (int j = 0; j < q.N; ++j) std::printf("INVTAB %s %d %d %.17g %d\n", tag, r, j, q.coeff(r, j), q.a_off[size_t(r ^ j)]);
    }
}

static int count_op(const gaast_program_desc& d, int opcode) {
    int c = 0;
    for (int i = 0; i < d.n_nodes; ++i) c += d.nodes[i].opcode == opcode;
    return c;
}
static int count_kind(const gaast_program_desc& d, int kind) {
    int c = 0;
    for (int i = 0; i < d.n_nodes; ++i) c += d.nodes[i].opcode == GAAST_OP_PRODUCT && d.nodes[i].product_kind == kind;
    return c;
}

static int count_steps(const gaast::Plan& plan, gaast::Step::Kind k) {
    int c = 0;
    for (const gaast::Step& s : plan.steps) c += s.kind == k;
    return c;
}

// lowers `d` under every plan form; supported: INVERSE steps expected (how many), else the plan must name what it cannot do
static void lower_all(const gaast_program_desc& d, const char* what, int want_inverse, bool supported) {
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
        CHECK(count_steps(plan, gaast::Step::INVERSE) == want_inverse);
        CHECK(plan.has_inverse == (want_inverse > 0));
        CHECK(count_steps(plan, gaast::Step::FUSED) == 0 || want_inverse == 0);   // an inverse is never part of a fused launch
        for (const gaast::Step& s : plan.steps)
            if (s.kind == gaast::Step::INVERSE) check_inverse_step(plan, s);
    }
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
            CHECK(a.nodes[i].child0 == b.nodes[i].child0 && a.nodes[i].minimal_grade_mask == b.nodes[i].minimal_grade_mask);
        }
        gaast_program_image_free(img);
    }
    for (size_t cut = 0; cut < need; cut += need / 5 + 1) CHECK(gaast_program_deserialize(buf.data(), cut) == nullptr);
}

// specialise, lower, serialise, differentiate with respect to every batched slot
// n_inv: INV nodes expected in the program (0: the scalar form); tab: print the lowered matrix under this tag
static void exercise(gaast_expr_t e, int n, const double* metric, const char* what, int n_inv, bool supported, const char* tab = nullptr) {
    gaast_spec_t spec = gaast_expr_specialize(e, n, metric, 0);
    if (!spec) std::printf("%s: %s\n", what, gaast_expr_last_error());
    CHECK(spec != nullptr);   // phases 1-3 succeed on the host for any n
    if (!spec) return;
    for (int dtype : {GAAST_F64, GAAST_F32}) {
        gaast_program_desc desc;
        CHECK(gaast_spec_program_desc(spec, dtype, 0, &desc) == 0);
        CHECK(count_op(desc, GAAST_OP_INV) == n_inv);
        for (int i = 0; i < desc.n_nodes; ++i)   // phase 3: the operand of an inverse is wanted in all of its grades
            if (desc.nodes[i].opcode == GAAST_OP_INV) {
                gaast_spec_node_info ci;
                CHECK(gaast_spec_node(spec, desc.nodes[i].child0, &ci) == 0);
                CHECK(desc.nodes[desc.nodes[i].child0].minimal_grade_mask == ci.maximal_grade_mask);
            }
        lower_all(desc, what, n_inv, supported);
        round_trip(desc);
        if (tab && dtype == GAAST_F64) {
            gaast::Plan plan;
            gaast::build_plan(desc, plan);
            print_inverse_steps(plan, tab);
        }
        for (int slot = 0; slot < desc.n_inputs; ++slot) {
            if (desc.inputs[slot].is_const) continue;
            gaast_program_image_t img = nullptr;
            const int st = gaast_program_vjp(&desc, slot, &img);
            if (st) std::printf("%s: vjp status %d: %s\n", what, st, gaast_expr_last_error());
            CHECK(st == 0 && img != nullptr);
            if (!img) continue;
            const gaast_program_desc& a = *gaast_program_image_desc(img);
            if (tab && dtype == GAAST_F64)
                std::printf("VJPOPS %s %d %d %d %d %d\n", tab, count_op(a, GAAST_OP_INV), count_kind(a, GAAST_PROD_GEOMETRIC + GAAST_PROD_ADJ_LEFT),
                            count_kind(a, GAAST_PROD_GEOMETRIC + GAAST_PROD_ADJ_RIGHT), count_op(a, GAAST_OP_NEG), count_op(a, GAAST_OP_PRODUCT));
            // the VJP program recomputes the inverse once per forward INV node on the path (here: every one)
            lower_all(a, what, count_op(a, GAAST_OP_INV), supported);
            round_trip(a);
            gaast_program_image_free(img);
        }
    }
    gaast_spec_free(spec);
    std::printf("ok  %s\n", what);
}

static uint64_t even_mask(int n) {
    uint64_t m = 0;
    for (int k = 0; k <= n; k += 2) m |= uint64_t(1) << k;
    return m;
}

int main() {
    const double pga[4] = {0, 1, 1, 1}, cga[5] = {1, 1, 1, 1, -1}, odd[3] = {2.0, -0.5, 1.0};
    double ones[GAAST_MAX_DIM];
    for (double& v : ones) v = 1.0;
    // full and even operands, n = 1 .. 8: N = 2^n / 2^(n-1) blades, refused beyond 64
    for (int n = 1; n <= 8; ++n) {
        const uint64_t full = (uint64_t(1) << (n + 1)) - 1;
        const std::string tf = "full" + std::to_string(n), te = "even" + std::to_string(n);
        exercise(H(gaast_expr_inv(H(gaast_expr_input(0, full, n)))), n, ones, ("inv(full) n=" + std::to_string(n)).c_str(), 1, n <= 6, n <= 3 ? tf.c_str() : nullptr);
        if (n >= 2)
            exercise(H(gaast_expr_inv(H(gaast_expr_input(0, even_mask(n), n)))), n, ones, ("inv(even) n=" + std::to_string(n)).c_str(), 1, n <= 7,
                     n <= 3 ? te.c_str() : nullptr);
    }
    // PGA3D (degenerate metric) full and even, CGA, a general diagonal metric: the matrices the host test compares with numpy
    exercise(H(gaast_expr_inv(H(gaast_expr_input(0, 0x1f, 4)))), 4, pga, "PGA3D inv(full)", 1, true, "pga-full");
    exercise(H(gaast_expr_inv(H(gaast_expr_input(0, 0x15, 4)))), 4, pga, "PGA3D inv(even)", 1, true, "pga-even");
    exercise(H(gaast_expr_inv(H(gaast_expr_input(0, 0x3f, 5)))), 5, cga, "CGA inv(full)", 1, true, "cga-full");
    exercise(H(gaast_expr_inv(H(gaast_expr_input(0, 0xf, 3)))), 3, odd, "inv(full) metric (2, -1/2, 1)", 1, true, "odd-full");
    // a mixed operand that lacks grades (vector + trivector): absent grades read as 0
    exercise(H(gaast_expr_inv(H(gaast_expr_input(0, 0xa, 4)))), 4, pga, "PGA3D inv(grades 1, 3)", 1, true, "pga-13");
    {   // the scalar form: ScalarInversion, no INV node, no INVERSE step
        exercise(H(gaast_expr_inv(H(gaast_expr_input(0, 1, 4)))), 4, pga, "inv(scalar input)", 0, true);
        exercise(H(gaast_expr_inv(H(gaast_expr_from_f64(2.5)))), 4, pga, "inv(2.5)", 0, true);
        gaast_spec_t spec = gaast_expr_specialize(H(gaast_expr_inv(H(gaast_expr_input(0, 1, 3)))), 3, ones, 0);
        CHECK(spec != nullptr);
        if (spec) {
            gaast_program_desc desc;
            CHECK(gaast_spec_program_desc(spec, GAAST_F64, 0, &desc) == 0);
            CHECK(count_op(desc, GAAST_OP_SINV) == 1 && count_op(desc, GAAST_OP_INV) == 0);
            // ... and the raw ABI carrying GAAST_OP_INV on a scalar: the same launches as GAAST_OP_SINV, and a VJP
            std::vector<gaast_node_desc> nodes(desc.nodes, desc.nodes + desc.n_nodes);
            gaast_program_desc raw = desc;
            for (gaast_node_desc& nd : nodes)
                if (nd.opcode == GAAST_OP_SINV) nd.opcode = GAAST_OP_INV;
            raw.nodes = nodes.data();
            for (uint32_t fl : {0u, uint32_t(GAAST_FLAG_NO_FUSION)}) {
                gaast_program_desc x = desc, y = raw;
                x.flags |= fl;
                y.flags |= fl;
                gaast::Plan p1, p2;
                gaast::build_plan(x, p1);
                gaast::build_plan(y, p2);
                CHECK(p1.error == GAAST_OK && p2.error == GAAST_OK && p2.unsupported.empty() && !p2.has_inverse);
                CHECK(p1.steps.size() == p2.steps.size());
                for (size_t i = 0; i < p1.steps.size() && i < p2.steps.size(); ++i) CHECK(p1.steps[i].kind == p2.steps[i].kind);
            }
            gaast_program_image_t i1 = nullptr, i2 = nullptr;
            CHECK(gaast_program_vjp(&desc, 0, &i1) == 0 && gaast_program_vjp(&raw, 0, &i2) == 0);
            if (i1 && i2) CHECK(gaast_program_image_desc(i1)->n_nodes == gaast_program_image_desc(i2)->n_nodes);
            gaast_program_image_free(i1);
            gaast_program_image_free(i2);
            gaast_spec_free(spec);
        }
        std::printf("ok  scalar forms\n");
    }
    {   // composition: wanted grades, an interior operand, sign-only arms over a bound input, products around the inverse
        gaast_expr_t a = H(gaast_expr_input(0, 0x1f, 4)), b = H(gaast_expr_input(1, 0x1f, 4)), c = H(gaast_expr_input(2, 0x1f, 4));
        exercise(H(gaast_expr_g(H(gaast_expr_inv(a)), 2)), 4, pga, "inv(a).g(2)", 1, true, "pga-g2");
        exercise(H(gaast_expr_product(H(gaast_expr_inv(H(gaast_expr_add(a, b)))), c, GAAST_PROD_GEOMETRIC)), 4, pga, "inv(a + b) * c", 1, true);
        exercise(H(gaast_expr_inv(H(gaast_expr_rev(a)))), 4, pga, "inv(~a)", 1, true, "pga-rev");
        exercise(H(gaast_expr_product(a, H(gaast_expr_inv(a)), GAAST_PROD_GEOMETRIC)), 4, pga, "a * inv(a)", 1, true);
        exercise(H(gaast_expr_inv(H(gaast_expr_inv(a)))), 4, pga, "inv(inv(a))", 2, true);
        exercise(H(gaast_expr_add(H(gaast_expr_inv(a)), b)), 4, pga, "inv(a) + b", 1, true);
        gaast_expr_t r = H(gaast_expr_input(0, 0x15, 6));
        exercise(H(gaast_expr_product(H(gaast_expr_inv(r)), H(gaast_expr_input(1, 0x2, 6)), GAAST_PROD_GEOMETRIC)), 6, ones, "inv(rotor) * v, n = 6", 1, true);
    }
    for (gaast_expr_t h : handles) gaast_expr_release(h);
    if (failures) {
        std::printf("%d CHECKS FAILED\n", failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
