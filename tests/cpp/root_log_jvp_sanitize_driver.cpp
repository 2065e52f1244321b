// Forward mode through the general square root and logarithm on the host, under AddressSanitizer + UBSan (CPU build only; no GPU, no
// HIP, never loaded into Python): gaast_program_vjp with and without GAAST_FLAG_GSQRT_GLOG_JVP through {GSQRT_ADJ, GSQRT_JVP} and
// {GLOG_ADJ, GLOG_JVP} (host/vjp.cpp: root_log_family_adjoint) and the lowering into Step::GSQRT_JVP / Step::GLOG_JVP (plan.cpp:
// lower_root_log_jvp) under every plan form, for n = 1 ... 7.  It also prints the tables of the lowered steps of hand-built programs
// ("RLOUT ..." / "RLTAB ..." lines) for tests/test_root_log_jvp_host.py to compare with numpy.
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

static bool is_jvp(gaast::Step::Kind k) { return k == gaast::Step::GSQRT_JVP || k == gaast::Step::GLOG_JVP; }

// every table of a GSQRT_JVP / GLOG_JVP step has its size, every offset stays inside the row it indexes, no result component is written
// twice, the right-multiplication words are those of L read at the other column, and both operand rows are in the list of the step's reads
static void check_step(const gaast::Plan& plan, const gaast::Step& s) {
    const gaast::Layout &la = plan.layout(s.a), &lr = plan.layout(s.res);
    const gaast::Step::Inverse& q = s.inv;
    CHECK(s.a.idx >= 0 && s.c.idx >= 0 && s.b.idx < 0);
    CHECK(!(s.a == s.res) && !(s.c == s.res));
    CHECK(q.N == 2 || q.N == 4 || q.N == 8 || q.N == 16 || q.N == 32 || q.N == 64);
    CHECK(q.N == (1 << (q.even ? plan.n - 1 : plan.n)));
    CHECK(q.blade.size() == size_t(q.N) && q.a_off.size() == size_t(q.N) && q.res_off.size() == size_t(q.N) && q.neg.size() == size_t(q.N));
    CHECK(q.h_off.size() == size_t(q.N) && q.rmul_neg.size() == size_t(q.N) && q.g_off.empty() && q.adj_neg_l.empty() && q.adj_neg_r.empty());
    CHECK(q.weight.size() == size_t(1) << plan.n && q.weight.size() <= 128);
    double wmax = 0;
    for (double w : q.weight) wmax = std::fmax(wmax, std::fabs(w));
    CHECK(q.wmax == wmax);
    if (q.h_off.size() != size_t(q.N) || q.rmul_neg.size() != size_t(q.N)) return;
    std::vector<char> seen(size_t(lr.row_len), 0);
    int produced = 0;
    for (int j = 0; j < q.N; ++j) {
        CHECK(q.a_off[size_t(j)] >= -1 && int64_t(q.a_off[size_t(j)]) < la.row_len);
        CHECK(q.res_off[size_t(j)] >= -1 && int64_t(q.res_off[size_t(j)]) < lr.row_len);
        CHECK(q.h_off[size_t(j)] >= -1 && int64_t(q.h_off[size_t(j)]) < plan.layout(s.c).row_len);
        if (q.res_off[size_t(j)] >= 0 && int64_t(q.res_off[size_t(j)]) < lr.row_len) {
            CHECK(!seen[size_t(q.res_off[size_t(j)])]);
            seen[size_t(q.res_off[size_t(j)])] = 1;
            ++produced;
        }
        for (int r = 0; r < q.N; ++r)   // R[r][j] = coeff(S[j], S[r] xor S[j]): the sign of L[r][r xor j]
            CHECK(((q.rmul_neg[size_t(r)] >> j) & 1ULL) == ((q.neg[size_t(r)] >> (r ^ j)) & 1ULL));
    }
    CHECK(produced == q.n_out && produced > 0);
    if (s.beta == 0) CHECK(int64_t(produced) == lr.row_len);
    if (q.N < 64) CHECK((q.a_neg >> q.N) == 0);
    int hits = 0;
    gaast::for_each_read(s, [&](gaast::BufRef r) { hits += (r == s.a) + (r == s.c); });
    CHECK(hits >= 2);
}

static void print_steps(const gaast::Plan& plan, const char* tag) {
    for (const gaast::Step& s : plan.steps) {
        if (!is_jvp(s.kind) && s.kind != gaast::Step::GSQRT_ADJ) continue;
        const gaast::Step::Inverse& q = s.inv;
        const char* kind = s.kind == gaast::Step::GSQRT_JVP ? "sqrt" : s.kind == gaast::Step::GLOG_JVP ? "log" : "sqrt_adj";
        for (int j = 0; j < q.N; ++j)
            std::printf("RLOUT %s %s %d %d %u %d %d %d %d\n", tag, kind, q.N, j, q.blade[size_t(j)], q.a_off[size_t(j)], q.res_off[size_t(j)],
                        is_jvp(s.kind) ? q.h_off[size_t(j)] : q.g_off[size_t(j)], int((q.a_neg >> j) & 1));
        if (!is_jvp(s.kind)) continue;
        for (int r = 0; r < q.N; ++r)
            for (int j = 0; j < q.N; ++j) {
                const double w = q.weight[size_t(q.blade[size_t(j)] & ~q.blade[size_t(r)])];
                std::printf("RLTAB %s %s %d %d %.17g %.17g\n", tag, kind, r, j, q.coeff(r, j), ((q.rmul_neg[size_t(r)] >> j) & 1ULL) ? -w : w);
            }
    }
}

// lowers `d` under every plan form: as many GSQRT_JVP / GLOG_JVP steps as nodes (at least: a node under a sign-only arm is evaluated
// once per buffer it is added into), each a launch of its own, none of them owning the domain-error counter
static void lower_all(const gaast_program_desc& d, const char* what, const char* tab = nullptr, bool supported = true) {
    const int n_sq = count_op(d, GAAST_OP_GSQRT_JVP), n_lg = count_op(d, GAAST_OP_GLOG_JVP);
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
        CHECK(count_steps(plan, gaast::Step::GSQRT_JVP) >= n_sq && count_steps(plan, gaast::Step::GLOG_JVP) >= n_lg);
        CHECK((n_sq > 0) == (count_steps(plan, gaast::Step::GSQRT_JVP) > 0) && (n_lg > 0) == (count_steps(plan, gaast::Step::GLOG_JVP) > 0));
        CHECK(plan.has_gsqrt == (count_steps(plan, gaast::Step::GSQRT) > 0) && plan.has_glog == (count_steps(plan, gaast::Step::GLOG) > 0));
        CHECK(count_steps(plan, gaast::Step::FUSED) == 0 || n_sq + n_lg == 0);
        for (const gaast::Step& s : plan.steps)
            if (is_jvp(s.kind)) check_step(plan, s);
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
        if (nd.opcode != GAAST_OP_GSQRT_JVP && nd.opcode != GAAST_OP_GLOG_JVP && nd.opcode != GAAST_OP_GSQRT_ADJ && nd.opcode != GAAST_OP_GLOG_ADJ) continue;
        CHECK(nd.child0 >= 0 && nd.child0 < i && nd.child1 >= 0 && nd.child1 < i && nd.input_slot == -1);
    }
}

static bool same_but_flags(const gaast_program_desc& a, const gaast_program_desc& b, uint32_t flag) {
    const size_t na = gaast_program_serialize(&a, nullptr, 0), nb = gaast_program_serialize(&b, nullptr, 0);
    if (na != nb || (a.flags ^ b.flags) != flag) return false;
    std::vector<unsigned char> x(na), y(nb);
    gaast_program_serialize(&a, x.data(), na);
    gaast_program_serialize(&b, y.data(), nb);
    int diff = 0;
    for (size_t i = 0; i < na; ++i) diff += x[i] != y[i];
    return diff == 1;
}

// first order in every batched slot with and without the flag (the same bytes but the flags word); second order in every batched
// slot of each image: without the flag refused in today's words; with it forward mode (the cotangent slot) holds exactly one tangent
// node, gsqrt differentiates in every slot and again (third order), glog is refused by name where its operand is on the path.
// `deep`: lower the third-order images too
static void exercise(gaast_expr_t e, int n, const double* metric, const char* what, bool log, bool supported, bool deep) {
    gaast_spec_t spec = gaast_expr_specialize(e, n, metric, 0);
    CHECK(spec != nullptr);
    if (!spec) return;
    const uint32_t FLAG = GAAST_FLAG_GSQRT_GLOG_JVP;
    const int op_adj = log ? GAAST_OP_GLOG_ADJ : GAAST_OP_GSQRT_ADJ, op_jvp = log ? GAAST_OP_GLOG_JVP : GAAST_OP_GSQRT_JVP;
    const char* adj_name = log ? "GAAST_OP_GLOG_ADJ" : "GAAST_OP_GSQRT_ADJ";
    int seen_jvp = 0, seen_operand = 0, refused = 0;
    for (int dtype : {GAAST_F64, GAAST_F32}) {
        gaast_program_desc plain, desc;
        CHECK(gaast_spec_program_desc(spec, dtype, 0, &plain) == 0);
        CHECK(gaast_spec_program_desc(spec, dtype, FLAG, &desc) == 0);
        CHECK(same_but_flags(plain, desc, FLAG));
        for (int s1 = 0; s1 < desc.n_inputs; ++s1) {
            if (desc.inputs[s1].is_const) continue;
            gaast_program_image_t i0 = nullptr, i1 = nullptr;
            CHECK(gaast_program_vjp(&plain, s1, &i0) == 0 && i0);
            CHECK(gaast_program_vjp(&desc, s1, &i1) == 0 && i1);
            if (!i0 || !i1) continue;
            const gaast_program_desc& a0 = *gaast_program_image_desc(i0);
            const gaast_program_desc& a = *gaast_program_image_desc(i1);
            CHECK(same_but_flags(a0, a, FLAG) && count_op(a, op_jvp) == 0);
            lower_all(a, what, nullptr, supported);
            const bool on_path = count_op(a, op_adj) > 0;
            for (int s2 = 0; s2 < a.n_inputs; ++s2) {
                if (a.inputs[s2].is_const) continue;
                gaast_program_image_t j0 = nullptr, i2 = nullptr;
                const int st0 = gaast_program_vjp(&a0, s2, &j0);   // without the flag
                if (st0) {
                    const std::string want = std::string("second-order reverse mode through ") + adj_name + " is not implemented";
                    CHECK(st0 == GAAST_ERR_UNIMPLEMENTED && want == gaast_expr_last_error() && on_path && !j0);
                }
                const int st = gaast_program_vjp(&a, s2, &i2);
                if (st) {   // glog alone, and only where the operand of a GLOG_ADJ node depends on the slot
                    CHECK(log && st0 == st && st == GAAST_ERR_UNIMPLEMENTED && !i2);
                    CHECK(std::strstr(gaast_expr_last_error(), adj_name) != nullptr && std::strstr(gaast_expr_last_error(), "with respect to its operand") != nullptr);
                    ++refused;
                    if (j0) gaast_program_image_free(j0);
                    continue;
                }
                CHECK(i2 != nullptr);
                if (!i2) continue;
                const gaast_program_desc& a2 = *gaast_program_image_desc(i2);
                if (st0 == 0 && j0) CHECK(same_but_flags(*gaast_program_image_desc(j0), a2, FLAG));   // the family is off the path: the same image
                if (j0) gaast_program_image_free(j0);
                seen_jvp += count_op(a2, op_jvp);
                if (st0 && s2 != a.n_inputs - 1 - (a.inputs[a.n_inputs - 1].is_const ? 1 : 0)) ++seen_operand;
                check_family_nodes(a2);
                lower_all(a2, what, nullptr, supported);
                round_trip(a2);
                for (int s3 = 0; s3 < a2.n_inputs; ++s3) {   // third order: gsqrt is closed; glog with respect to the tangent path only
                    if (a2.inputs[s3].is_const) continue;
                    gaast_program_image_t i3 = nullptr;
                    const int st3 = gaast_program_vjp(&a2, s3, &i3);
                    if (st3) {
                        CHECK(log && st3 == GAAST_ERR_UNIMPLEMENTED && std::strstr(gaast_expr_last_error(), "with respect to its operand") != nullptr);
                    } else if (i3) {
                        check_family_nodes(*gaast_program_image_desc(i3));
                        if (deep && dtype == GAAST_F64) lower_all(*gaast_program_image_desc(i3), what, nullptr, supported);
                        gaast_program_image_free(i3);
                    }
                }
                gaast_program_image_free(i2);
            }
            gaast_program_image_free(i0);
            gaast_program_image_free(i1);
        }
    }
    CHECK(seen_jvp > 0);
    if (log) CHECK(refused > 0 && seen_operand == 0);
    else CHECK(refused == 0 && seen_operand > 0);
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
    for (int n = 1; n <= 7; ++n) {   // gsqrt(x) and glog(x) over every blade (n <= 6) and over the even blades (n >= 2); n = 7 full: beyond the kernels
        const uint64_t full = (uint64_t(2) << n) - 1, even = full & 0x5555555555555555ULL;
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 1 && n == 1) continue;
            const uint64_t mask = pass ? even : full;
            const bool supported = pass ? n <= 7 : n <= 6;
            const std::string tag = std::string(pass ? "even" : "full") + " n=" + std::to_string(n);
            gaast_expr_t x = H(gaast_expr_input(0, mask, n));
            exercise(H(gaast_expr_gsqrt(x)), n, ones, ("gsqrt(x) " + tag).c_str(), false, supported, n <= 4);
            exercise(H(gaast_expr_glog(x)), n, ones, ("glog(x) " + tag).c_str(), true, supported, n <= 4);
        }
    }
    {
        gaast_expr_t x = H(gaast_expr_input(0, 0x5, 3)), y = H(gaast_expr_input(1, 0x5, 3));
        exercise(H(gaast_expr_product(H(gaast_expr_gsqrt(x)), y, GAAST_PROD_GEOMETRIC)), 3, ones, "gsqrt(x) * y", false, true, true);
        gaast_expr_t m = H(gaast_expr_input(0, 0x15, 4)), t = H(gaast_expr_input(1, 0x15, 4));
        exercise(H(gaast_expr_glog(H(gaast_expr_product(m, H(gaast_expr_inv(t)), GAAST_PROD_GEOMETRIC)))), 4, pga, "glog(m * t.inv())", true, true, true);
        exercise(H(gaast_expr_gsqrt(H(gaast_expr_product(m, H(gaast_expr_rev(t)), GAAST_PROD_GEOMETRIC)))), 4, pga, "gsqrt(m ~t)", false, true, true);
    }
    {   // the tables the host test compares with numpy: the tangent holds a part of the blade set, the result another, the operand is
        // read through a reverse (grade 2 and 3 negated in the read)
        for (int kind = 0; kind < 2; ++kind) {
            const int op = kind ? GAAST_OP_GLOG_JVP : GAAST_OP_GSQRT_JVP;
            Raw p;   // PGA3D: every blade
            const int hp = p.input(0x0e, 4), bp = p.input(0x1f, 4);
            const int ap = p.node(GAAST_OP_REVERSE, bp, -1, -1, 0x1f, 4);
            p.node(op, hp, ap, -1, 0x17, 4);
            lower_all(p.desc(4, pga), "raw tangent, PGA3D", "pga");
            round_trip(p.d);
            Raw c;   // CGA: the even blades from a bivector operand, the tangent a scalar and a 4-vector
            const int hc = c.input(0x11, 5), ac = c.input(0x4, 5);
            c.node(op, hc, ac, -1, 0x15, 5);
            lower_all(c.desc(5, cga), "raw tangent, CGA", "cga");
            round_trip(c.d);
            Raw o;   // a metric (2, -1/2, 1): the metric factors
            const int ho = o.input(0xf, 3), ao = o.input(0xf, 3);
            o.node(op, ho, ao, -1, 0xf, 3);
            lower_all(o.desc(3, odd), "raw tangent, metric (2, -1/2, 1)", "odd");
        }
        Raw f;   // a GSQRT_ADJ node with the mask of the whole blade set over a bivector operand: every blade is produced
        const int gf = f.input(0x15, 4), af = f.input(0x4, 4);
        f.node(GAAST_OP_GSQRT_ADJ, gf, af, -1, 0x15, 4);
        lower_all(f.desc(4, pga), "raw GSQRT_ADJ, whole blade set", "adj-full");
        Raw gl;  // ... where GLOG_ADJ keeps the restriction to the operand's grades
        const int gg = gl.input(0x15, 4), ag = gl.input(0x4, 4);
        gl.node(GAAST_OP_GLOG_ADJ, gg, ag, -1, 0x15, 4);
        gaast::Plan pl;
        gaast::build_plan(gl.desc(4, pga), pl);
        CHECK(pl.error == GAAST_OK && count_steps(pl, gaast::Step::GLOG_ADJ) == 1);
        for (const gaast::Step& s : pl.steps)
            if (s.kind == gaast::Step::GLOG_ADJ) CHECK(s.inv.n_out == 6);
        std::printf("ok  raw tables\n");
    }
    {   // malformed nodes of the raw ABI are refused, not read out of bounds
        for (int op : {GAAST_OP_GSQRT_JVP, GAAST_OP_GLOG_JVP}) {
            Raw j;   // a tangent with a grade outside the blade set
            const int h = j.input(0x2, 3), a = j.input(0x4, 3);
            j.node(op, h, a, -1, 0x5, 3);
            gaast::Plan plan;
            gaast::build_plan(j.desc(3, ones), plan);
            CHECK(plan.error == GAAST_ERR_INVALID_PROGRAM);
            for (int c1 : {-1, 2, 9}) {   // the operand must be an earlier node
                Raw m;
                const int h3 = m.input(0x5, 3);
                m.input(0x5, 3);
                m.node(op, h3, c1, -1, 0x5, 3);
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
            big.node(op, hb, ab, -1, 0xff, 7);
            gaast::Plan pb;
            gaast::build_plan(big.desc(7, ones), pb);
            CHECK(pb.error == GAAST_OK && !pb.unsupported.empty());
        }
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
