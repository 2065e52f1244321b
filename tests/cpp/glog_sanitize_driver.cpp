// The general multivector logarithm on the host, under AddressSanitizer + UBSan (CPU build only; no GPU, no HIP, never loaded into
// Python): grade inference and the phase-3 restriction (host/expr.cpp), the wire format, gaast_program_vjp through GAAST_OP_GLOG
// (host/vjp.cpp: one GAAST_OP_GLOG_ADJ node) and the lowering into Step::GLOG / Step::GLOG_ADJ (plan.cpp: lower_gexp,
// lower_gexp_adj, which lower both functions) for n = 1 ... 8, full and even operands, under every plan form.
// It also prints the tables of the lowered steps ("GLOGOUT ..." / "GLOGTAB ..." / "ADJTAB ..." lines) for tests/test_glog_host.py
// to compare with numpy, and the census of the VJP programs ("VJPOPS ..." lines).
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

// every table of a GLOG / GLOG_ADJ step has its size, every offset stays inside the row it indexes, no result component is written
// twice, every index the kernels form stays inside the table it reads
static void check_glog_step(const gaast::Plan& plan, const gaast::Step& s) {
    const bool adj = s.kind == gaast::Step::GLOG_ADJ;
    const gaast::Layout &la = plan.layout(s.a), &lr = plan.layout(s.res);
    const gaast::Step::Inverse& q = s.inv;
    CHECK(!(s.a == s.res));
    CHECK(q.N == 2 || q.N == 4 || q.N == 8 || q.N == 16 || q.N == 32 || q.N == 64);
    CHECK(q.N == (1 << (q.even ? plan.n - 1 : plan.n)));
    CHECK(q.blade.size() == size_t(q.N) && q.a_off.size() == size_t(q.N) && q.res_off.size() == size_t(q.N) && q.neg.size() == size_t(q.N));
    CHECK(q.weight.size() == size_t(1) << plan.n && q.weight.size() <= 128);
    double wmax = 0;
    for (double w : q.weight) wmax = std::fmax(wmax, std::fabs(w));
    CHECK(q.wmax == wmax);
    if (adj) {
        CHECK(s.b.idx >= 0 && !(s.b == s.res));
        CHECK(q.g_off.size() == size_t(q.N) && q.adj_neg_l.size() == size_t(q.N) && q.adj_neg_r.size() == size_t(q.N));
    } else {
        CHECK(q.g_off.empty() && q.adj_neg_l.empty() && q.adj_neg_r.empty());
    }
    std::vector<char> seen(size_t(lr.row_len), 0);
    int produced = 0;
    for (int j = 0; j < q.N && size_t(j) < q.blade.size(); ++j) {
        CHECK(q.blade[size_t(j)] < (1u << plan.n));
        if (j) CHECK(q.blade[size_t(j)] > q.blade[size_t(j - 1)]);
        CHECK(q.a_off[size_t(j)] >= -1 && int64_t(q.a_off[size_t(j)]) < la.row_len);
        CHECK(q.res_off[size_t(j)] >= -1 && int64_t(q.res_off[size_t(j)]) < lr.row_len);
        if (adj && size_t(j) < q.g_off.size()) CHECK(q.g_off[size_t(j)] >= -1 && int64_t(q.g_off[size_t(j)]) < plan.layout(s.b).row_len);
        if (q.res_off[size_t(j)] >= 0 && int64_t(q.res_off[size_t(j)]) < lr.row_len) {
            CHECK(!seen[size_t(q.res_off[size_t(j)])]);
            seen[size_t(q.res_off[size_t(j)])] = 1;
            ++produced;
            if (adj) CHECK(q.a_off[size_t(j)] >= 0);   // the cotangent is restricted to what the operand holds
        }
        for (int r = 0; r < q.N; ++r) {
            uint32_t x = q.blade[size_t(r)] ^ q.blade[size_t(j)];
            CHECK((q.even ? x >> 1 : x) == uint32_t(r ^ j));
            // the kernels' index arithmetic: S[j] & ~S[r] and S[r] & S[j] from the indices alone
            const uint32_t e = uint32_t(q.even), pj = uint32_t(__builtin_popcount(uint32_t(j))) & 1u, pr = uint32_t(__builtin_popcount(uint32_t(r))) & 1u;
            CHECK((((uint32_t(j) & ~uint32_t(r)) << e) | (e & pj & ~pr & 1u)) == (q.blade[size_t(j)] & ~q.blade[size_t(r)]));
            CHECK((((uint32_t(j) & uint32_t(r)) << e) | (e & pj & pr)) == (q.blade[size_t(j)] & q.blade[size_t(r)]));
            if (adj && q.adj_neg_l.size() == size_t(q.N) && q.adj_neg_r.size() == size_t(q.N)) {   // a = r, b = j: the sign of L[a xor b][b]
                const uint64_t want = (q.neg[size_t(r ^ j)] >> j) & 1ULL;
                CHECK(((q.adj_neg_l[size_t(r)] >> j) & 1ULL) == want && ((q.adj_neg_r[size_t(j)] >> r) & 1ULL) == want);
            }
        }
    }
    CHECK(produced == q.n_out && produced > 0);
    if (s.beta == 0) CHECK(int64_t(produced) == lr.row_len);
    if (q.N < 64) CHECK((q.a_neg >> q.N) == 0);
}

static void print_steps(const gaast::Plan& plan, const char* tag) {
    for (const gaast::Step& s : plan.steps) {
        const gaast::Step::Inverse& q = s.inv;
        if (s.kind == gaast::Step::GLOG) {
            for (int j = 0; j < q.N; ++j)
                std::printf("GLOGOUT %s %d %d %u %d %d %d %.17g\n", tag, q.N, j, q.blade[size_t(j)], q.a_off[size_t(j)], q.res_off[size_t(j)], int((q.a_neg >> j) & 1), q.wmax);
            for (int r = 0; r < q.N; ++r)
                for (int j = 0; j < q.N; ++j) std::printf("GLOGTAB %s %d %d %.17g\n", tag, r, j, q.coeff(r, j));
        } else if (s.kind == gaast::Step::GLOG_ADJ) {
            for (int a = 0; a < q.N; ++a)
                for (int b = 0; b < q.N; ++b) {
                    const double w = q.weight[size_t(q.blade[size_t(a)] & q.blade[size_t(b)])];
                    std::printf("ADJTAB %s %d %d %.17g %.17g %d %d\n", tag, a, b, ((q.adj_neg_l[size_t(a)] >> b) & 1ULL) ? -w : w,
                                ((q.adj_neg_r[size_t(b)] >> a) & 1ULL) ? -w : w, q.g_off[size_t(a)], q.res_off[size_t(a)]);
                }
        }
    }
}

// the steps of the three older functions over the same blade sets, for the host test to see that their tables are what they were
static void print_old_steps(gaast_expr_t e, int n, const double* metric, const char* kind, const char* tag) {
    gaast_spec_t spec = gaast_expr_specialize(e, n, metric, 0);
    CHECK(spec != nullptr);
    if (!spec) return;
    gaast_program_desc desc;
    CHECK(gaast_spec_program_desc(spec, GAAST_F64, 0, &desc) == 0);
    gaast::Plan plan;
    gaast::build_plan(desc, plan);
    CHECK(plan.error == GAAST_OK && plan.unsupported.empty() && plan.has_glog == 0);
    for (const gaast::Step& s : plan.steps) {
        if (s.kind != gaast::Step::INVERSE && s.kind != gaast::Step::GEXP && s.kind != gaast::Step::GSQRT) continue;
        const gaast::Step::Inverse& q = s.inv;
        for (int j = 0; j < q.N; ++j)
            std::printf("OLDOUT %s %s %d %u %d %d %d\n", kind, tag, j, q.blade[size_t(j)], q.a_off[size_t(j)], q.res_off[size_t(j)], int((q.a_neg >> j) & 1));
        for (int r = 0; r < q.N; ++r)
            for (int j = 0; j < q.N; ++j) std::printf("OLDTAB %s %s %d %d %.17g\n", kind, tag, r, j, q.coeff(r, j));
    }
    gaast_spec_free(spec);
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

// lowers `d` under every plan form; supported: GLOG / GLOG_ADJ steps expected (how many), else the plan must name what it cannot do
// (exact_steps false: a logarithm under a sign-only arm is evaluated once per buffer it is added into, as every arm is)
static void lower_all(const gaast_program_desc& d, const char* what, int want_glog, int want_adj, bool supported, const char* tab = nullptr, bool exact_steps = true) {
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
        if (exact_steps) CHECK(count_steps(plan, gaast::Step::GLOG) == want_glog && count_steps(plan, gaast::Step::GLOG_ADJ) == want_adj);
        else CHECK(count_steps(plan, gaast::Step::GLOG) >= want_glog && count_steps(plan, gaast::Step::GLOG_ADJ) >= want_adj);
        CHECK(plan.has_glog == (want_glog > 0));
        CHECK(count_steps(plan, gaast::Step::FUSED) == 0 || want_glog + want_adj == 0);   // never part of a fused launch
        for (const gaast::Step& s : plan.steps) {
            if (s.kind == gaast::Step::GLOG || s.kind == gaast::Step::GLOG_ADJ) check_glog_step(plan, s);
            if (s.kind == gaast::Step::GLOG_ADJ) {   // both rows are in the one list of a step's reads
                int hits = 0;
                gaast::for_each_read(s, [&](gaast::BufRef r) { hits += (r == s.a) + (r == s.b); });
                CHECK(hits >= 2);
            }
        }
        if (tab && extra == 0) print_steps(plan, tab);
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
            if (a.nodes[i].opcode == GAAST_OP_GLOG_ADJ) CHECK(a.nodes[i].child1 == b.nodes[i].child1 && b.nodes[i].child1 >= 0);
        }
        gaast_program_image_free(img);
    }
    for (size_t cut = 0; cut < need; cut += need / 5 + 1) CHECK(gaast_program_deserialize(buf.data(), cut) == nullptr);
}

// specialise, lower, serialise, differentiate with respect to every batched slot
static void exercise(gaast_expr_t e, int n, const double* metric, const char* what, int n_glog, bool supported, const char* tab = nullptr, bool exact_steps = true) {
    gaast_spec_t spec = gaast_expr_specialize(e, n, metric, 0);
    if (!spec) std::printf("%s: %s\n", what, gaast_expr_last_error());
    CHECK(spec != nullptr);   // phases 1-3 succeed on the host for any n
    if (!spec) return;
    for (int dtype : {GAAST_F64, GAAST_F32}) {
        gaast_program_desc desc;
        CHECK(gaast_spec_program_desc(spec, dtype, 0, &desc) == 0);
        CHECK(count_op(desc, GAAST_OP_GLOG) == n_glog);
        for (int i = 0; i < desc.n_nodes; ++i)   // phase 3: the operand is wanted in all of its grades
            if (desc.nodes[i].opcode == GAAST_OP_GLOG) {
                gaast_spec_node_info ci;
                CHECK(gaast_spec_node(spec, desc.nodes[i].child0, &ci) == 0);
                CHECK(desc.nodes[desc.nodes[i].child0].minimal_grade_mask == ci.maximal_grade_mask);
            }
        lower_all(desc, what, n_glog, 0, supported, dtype == GAAST_F64 ? tab : nullptr, exact_steps);
        round_trip(desc);
        for (int slot = 0; slot < desc.n_inputs; ++slot) {
            if (desc.inputs[slot].is_const) continue;
            gaast_program_image_t img = nullptr;
            const int st = gaast_program_vjp(&desc, slot, &img);
            if (st) std::printf("%s: vjp status %d: %s\n", what, st, gaast_expr_last_error());
            CHECK(st == 0 && img != nullptr);
            if (!img) continue;
            const gaast_program_desc& a = *gaast_program_image_desc(img);
            if (tab && dtype == GAAST_F64) {
                std::printf("VJPOPS %s %d %d %d %d\n", tab, slot, a.n_nodes, count_op(a, GAAST_OP_GLOG_ADJ), count_op(a, GAAST_OP_GLOG));
                for (int i = 0; i < a.n_nodes; ++i)
                    if (a.nodes[i].opcode == GAAST_OP_GLOG_ADJ)
                        std::printf("VJPADJ %s %d %d %d %d %d %llu\n", tab, slot, a.nodes[a.nodes[i].child0].opcode, a.nodes[a.nodes[i].child0].input_slot,
                                    a.nodes[a.nodes[i].child1].opcode, a.nodes[a.nodes[i].child1].input_slot, (unsigned long long)a.nodes[i].minimal_grade_mask);
            }
            lower_all(a, what, count_op(a, GAAST_OP_GLOG), count_op(a, GAAST_OP_GLOG_ADJ), supported, dtype == GAAST_F64 ? tab : nullptr, exact_steps);
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
    // full and even operands, n = 1 .. 8: N = 2^n / 2^(n-1) blades, refused beyond 64; the even operand at n = 1 is a bare scalar
    // over a one-blade set: there is no scalar lowering, the GLOG node stays and the plan names what the back end cannot do
    for (int n = 1; n <= 8; ++n) {
        const uint64_t full = (uint64_t(1) << (n + 1)) - 1;
        const std::string tf = "full" + std::to_string(n), te = "even" + std::to_string(n);
        exercise(H(gaast_expr_glog(H(gaast_expr_input(0, full, n)))), n, ones, ("glog(full) n=" + std::to_string(n)).c_str(), 1, n <= 6, n <= 3 ? tf.c_str() : nullptr);
        exercise(H(gaast_expr_glog(H(gaast_expr_input(0, even_mask(n), n)))), n, ones, ("glog(even) n=" + std::to_string(n)).c_str(), 1, n >= 2 && n <= 7,
                 n == 2 || n == 3 ? te.c_str() : nullptr);
    }
    exercise(H(gaast_expr_glog(H(gaast_expr_input(0, 1, 0)))), 0, ones, "glog(scalar) n=0", 1, false);
    exercise(H(gaast_expr_glog(H(gaast_expr_input(0, 1, 3)))), 3, ones, "glog(scalar) n=3", 1, true);   // a scalar operand is evaluated over the even set
    // PGA3D (degenerate metric) bivectors and full, CGA, a general diagonal metric: the tables the host test compares with numpy
    exercise(H(gaast_expr_glog(H(gaast_expr_input(0, 0x4, 4)))), 4, pga, "PGA3D glog(bivector)", 1, true, "pga-biv");
    exercise(H(gaast_expr_glog(H(gaast_expr_input(0, 0x1f, 4)))), 4, pga, "PGA3D glog(full)", 1, true, "pga-full");
    exercise(H(gaast_expr_glog(H(gaast_expr_input(0, 0x4, 5)))), 5, cga, "CGA glog(bivector)", 1, true, "cga-biv");
    exercise(H(gaast_expr_glog(H(gaast_expr_input(0, 0xf, 3)))), 3, odd, "glog(full) metric (2, -1/2, 1)", 1, true, "odd-full");
    exercise(H(gaast_expr_glog(H(gaast_expr_input(0, 0xa, 4)))), 4, pga, "PGA3D glog(grades 1, 3)", 1, true, "pga-13");
    print_old_steps(H(gaast_expr_inv(H(gaast_expr_input(0, 0x1f, 4)))), 4, pga, "INV", "pga-full");
    print_old_steps(H(gaast_expr_gexp(H(gaast_expr_input(0, 0x1f, 4)))), 4, pga, "GEXP", "pga-full");
    print_old_steps(H(gaast_expr_inv(H(gaast_expr_input(0, 0x4, 5)))), 5, cga, "INV", "cga-biv");
    print_old_steps(H(gaast_expr_gexp(H(gaast_expr_input(0, 0x4, 5)))), 5, cga, "GEXP", "cga-biv");
    print_old_steps(H(gaast_expr_inv(H(gaast_expr_input(0, 0xf, 3)))), 3, odd, "INV", "odd-full");
    print_old_steps(H(gaast_expr_gexp(H(gaast_expr_input(0, 0xf, 3)))), 3, odd, "GEXP", "odd-full");
    print_old_steps(H(gaast_expr_gsqrt(H(gaast_expr_input(0, 0x1f, 4)))), 4, pga, "GSQRT", "pga-full");
    print_old_steps(H(gaast_expr_gsqrt(H(gaast_expr_input(0, 0x4, 5)))), 5, cga, "GSQRT", "cga-biv");
    print_old_steps(H(gaast_expr_gsqrt(H(gaast_expr_input(0, 0xf, 3)))), 3, odd, "GSQRT", "odd-full");
    {   // composition: wanted grades, an interior operand, sign-only arms over a bound input, products around the exponential
        gaast_expr_t a = H(gaast_expr_input(0, 0x1f, 4)), b = H(gaast_expr_input(1, 0x1f, 4)), c = H(gaast_expr_input(2, 0x1f, 4));
        gaast_expr_t B = H(gaast_expr_input(0, 0x4, 4)), X = H(gaast_expr_input(1, 0x8, 4));
        exercise(H(gaast_expr_g(H(gaast_expr_glog(a)), 2)), 4, pga, "glog(a).g(2)", 1, true, "pga-g2");
        exercise(H(gaast_expr_product(H(gaast_expr_glog(H(gaast_expr_add(a, b)))), c, GAAST_PROD_GEOMETRIC)), 4, pga, "glog(a + b) * c", 1, true);
        exercise(H(gaast_expr_glog(H(gaast_expr_rev(B)))), 4, pga, "glog(~B)", 1, true, "pga-rev");
        exercise(H(gaast_expr_glog(H(gaast_expr_glog(B)))), 4, pga, "glog(glog(B))", 2, true);
        exercise(H(gaast_expr_add(H(gaast_expr_glog(a)), b)), 4, pga, "glog(a) + b", 1, true);
        gaast_expr_t R = H(gaast_expr_glog(B));
        exercise(H(gaast_expr_product(H(gaast_expr_product(R, X, GAAST_PROD_GEOMETRIC)), H(gaast_expr_rev(R)), GAAST_PROD_GEOMETRIC)), 4, pga, "glog(B) X ~glog(B)", 1, true, nullptr, false);
        exercise(H(gaast_expr_product(H(gaast_expr_glog(B)), H(gaast_expr_glog(H(gaast_expr_neg(B)))), GAAST_PROD_GEOMETRIC)), 4, pga, "glog(B) glog(-B)", 2, true);
    }
    {   // N = 1 is reachable through the raw ABI alone: a GLOG node over a bare scalar at n = 1 (the even set has one blade) lowers
        // without an error and the plan names what the back end cannot do; at n = 3 the same node is the 4-blade even logarithm
        gaast_node_desc nodes[2] = {};
        for (gaast_node_desc& nd : nodes) { nd.child0 = nd.child1 = -1; nd.input_slot = -1; nd.product_kind = GAAST_PROD_EXPLICIT; }
        gaast_input_desc ins[1] = {{0x1, 1, 0, nullptr}};
        for (int n : {1, 3}) {
            nodes[0].opcode = GAAST_OP_INPUT; nodes[0].input_slot = 0; nodes[0].minimal_grade_mask = 0x1; nodes[0].vec_space_dim = n;
            nodes[1].opcode = GAAST_OP_GLOG; nodes[1].child0 = 0; nodes[1].minimal_grade_mask = 0x1; nodes[1].vec_space_dim = n;
            ins[0].storage_dim = n;
            gaast_program_desc d{};
            d.vec_space_dim = n; d.metric_diag = ones; d.dtype = GAAST_F64; d.n_inputs = 1; d.inputs = ins; d.n_nodes = 2; d.nodes = nodes; d.root = 1;
            gaast::Plan plan;
            gaast::build_plan(d, plan);
            CHECK(plan.error == GAAST_OK);
            CHECK(plan.unsupported.empty() == (n == 3));
            if (n == 3) CHECK(count_steps(plan, gaast::Step::GLOG) == 1 && plan.has_glog == 1);
        }
        std::printf("ok  raw GLOG node over a scalar\n");
    }
    {   // malformed adjoint nodes of the raw ABI are refused, not read out of bounds: a cotangent outside the blade set
        gaast_node_desc nodes[3] = {};
        for (gaast_node_desc& nd : nodes) { nd.child0 = nd.child1 = -1; nd.input_slot = -1; nd.vec_space_dim = 3; nd.product_kind = GAAST_PROD_EXPLICIT; }
        nodes[0].opcode = GAAST_OP_INPUT; nodes[0].input_slot = 0; nodes[0].minimal_grade_mask = 0x2;   // g: a vector
        nodes[1].opcode = GAAST_OP_INPUT; nodes[1].input_slot = 1; nodes[1].minimal_grade_mask = 0x4;   // A: a bivector (even set)
        nodes[2].opcode = GAAST_OP_GLOG_ADJ; nodes[2].child0 = 0; nodes[2].child1 = 1; nodes[2].minimal_grade_mask = 0x4;
        gaast_input_desc ins[2] = {{0x2, 3, 0, nullptr}, {0x4, 3, 0, nullptr}};
        gaast_program_desc d{};
        d.vec_space_dim = 3; d.metric_diag = ones; d.dtype = GAAST_F64; d.n_inputs = 2; d.inputs = ins; d.n_nodes = 3; d.nodes = nodes; d.root = 2;
        gaast::Plan plan;
        gaast::build_plan(d, plan);
        CHECK(plan.error == GAAST_ERR_INVALID_PROGRAM);
        nodes[0].minimal_grade_mask = 0x5; ins[0].grade_mask = 0x5;   // within the even set: lowers
        gaast::Plan ok;
        gaast::build_plan(d, ok);
        CHECK(ok.error == GAAST_OK && ok.unsupported.empty() && count_steps(ok, gaast::Step::GLOG_ADJ) == 1);
        std::printf("ok  raw adjoint nodes\n");
    }
    for (gaast_expr_t h : handles) gaast_expr_release(h);
    if (failures) {
        std::printf("%d CHECKS FAILED\n", failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
