// CPU-only: the launch-time forms of k_gp_mfma32p<false, 12, *, *> follow the plan's maps.  The dense launcher (runtime.hip: run_dense)
// passes Step::Dense::left_signs / right_signs and plan.hpp's dense_whole_row_stores(step) to the kernel, which then stages a side
// without the sign xor and writes each result with one store at a lane-constant offset.  A flag that says more than its map words do
// gives wrong results without any fault, so every flag is recomputed here from the words of the maps of plans built by
// gaast::build_plan, for R^12 f32 programs:
//   full       a * b, Euclidean: whole rows, no sign bit on the left; the right map carries the signs of the B image (so that flag is set)
//   projected  (a * b).g(6): blades without a place in the result row (out_map words -1): no whole rows
//   signed     a * b with -1 on vectors 0 and 7: the permuted basis reorders blades, out_map words carry signs: no whole rows
//   reversed   a.rev() * b: the reversion is folded into the left map as sign bits: left_signs
//   sum        a * b + c * d: the second product accumulates (beta = 1): no whole rows for it, whole rows for the first
// Build: g++ -std=c++17 -O1 -fsanitize=address,undefined -I include -I gaast_amd/csrc/device -I gaast_amd/csrc/common -I gaast_amd/csrc/host
//        tests/cpp/dense_flags_driver.cpp + tests/helpers.py: plan_sources
#include <cstdio>
#include <string>
#include <vector>

#include "gaast_expr.h"
#include "plan.hpp"

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("FAIL %s: ", #cond);               \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
            g_fail = 1;                                    \
        }                                                  \
    } while (0)

struct Flags {
    int whole, left_signs, right_signs, beta;
};

// the dense steps of the program, each with its flags checked against the words of its maps
static std::vector<Flags> dense_flags(const char* what, gaast_expr_t e, int n, const std::vector<double>& metric) {
    std::vector<Flags> out;
    gaast_spec_t spec = gaast_expr_specialize(e, n, metric.data(), uint64_t(1) << 22);
    gaast_program_desc desc;
    if (!spec || gaast_spec_program_desc(spec, GAAST_F32, 0, &desc) != 0) {
        std::printf("FAIL %s: no program: %s\n", what, gaast_expr_last_error());
        g_fail = 1;
        return out;
    }
    gaast::Plan plan;
    gaast::build_plan(desc, plan, false, false);
    for (const gaast::Step& s : plan.steps) {
        if (s.kind != gaast::Step::PRODUCT_DENSE) continue;
        const gaast::Step::Dense& q = s.dense;
        CHECK(q.family == gaast::DenseFamily::MFMA32P && q.n == 12 && !q.degenerate, "%s: family %d n %d", what, int(q.family), q.n);
        int lneg = 0, rneg = 0, absent = 0, osign = 0;
        for (uint32_t w : q.left_map) lneg |= int(w >> 31);
        for (uint32_t w : q.right_map) rneg |= int(w >> 31);
        for (int32_t w : q.out_map) {
            absent |= int(w < 0);
            osign |= int(w >= 0 && (uint32_t(w) & 0x40000000u));
        }
        CHECK(q.out_map.size() == size_t(1) << 12, "%s: %zu out_map words", what, q.out_map.size());
        CHECK(q.left_signs == lneg, "%s: left_signs %d, map words %d", what, q.left_signs, lneg);
        CHECK(q.right_signs == rneg, "%s: right_signs %d, map words %d", what, q.right_signs, rneg);
        CHECK(q.out_signs == osign, "%s: out_signs %d, map words %d", what, q.out_signs, osign);
        CHECK(q.out_all == !absent, "%s: out_all %d, absent words %d", what, q.out_all, absent);
        const bool whole = gaast::dense_whole_row_stores(s);
        CHECK(whole == (!absent && !osign && s.beta == 0 && q.out_scale.empty() && !q.scaled), "%s: whole rows %d with absent %d signs %d beta %d scaled %d",
              what, int(whole), absent, osign, s.beta, q.scaled);
        // whole rows write 16 words per lane without looking at them: each must be a plain offset inside a row of 4096 * 4 bytes at most
        if (whole)
            for (int32_t w : q.out_map) CHECK(w >= 0 && w < (1 << 12), "%s: out_map word %d on the whole-row path", what, w);
        out.push_back(Flags{int(whole), q.left_signs, q.right_signs, s.beta});
        std::printf("%s: %s | whole_rows=%d left_signs=%d right_signs=%d out_signs=%d out_all=%d beta=%d\n", what, s.name.c_str(), int(whole), q.left_signs,
                    q.right_signs, q.out_signs, q.out_all, s.beta);
    }
    gaast_spec_free(spec);
    return out;
}

int main() {
    const int n = 12;
    const uint64_t full = (uint64_t(2) << n) - 1;
    constexpr int GP = GAAST_PROD_GEOMETRIC;
    const std::vector<double> euclid(size_t(n), 1.0);
    std::vector<double> mixed = euclid;
    mixed[0] = mixed[7] = -1.0;
    std::vector<gaast_expr_t> handles;   // every expression handle is released at the end
    auto keep = [&](gaast_expr_t e) {
        handles.push_back(e);
        return e;
    };
    auto in = [&](int slot) { return keep(gaast_expr_input(slot, full, n)); };
    auto mul = [&](gaast_expr_t a, gaast_expr_t b) { return keep(gaast_expr_product(a, b, GP)); };

    std::vector<Flags> f = dense_flags("full", mul(in(0), in(1)), n, euclid);
    CHECK(f.size() == 1 && f[0].whole == 1 && f[0].left_signs == 0 && f[0].right_signs == 1 && f[0].beta == 0, "full: %zu dense steps", f.size());

    f = dense_flags("projected", keep(gaast_expr_g(mul(in(0), in(1)), 6)), n, euclid);
    CHECK(f.size() == 1 && f[0].whole == 0 && f[0].left_signs == 0, "projected: %zu dense steps", f.size());

    f = dense_flags("signed", mul(in(0), in(1)), n, mixed);
    CHECK(f.size() == 1 && f[0].whole == 0, "signed: %zu dense steps", f.size());

    f = dense_flags("reversed", mul(keep(gaast_expr_rev(in(0))), in(1)), n, euclid);
    CHECK(f.size() == 1 && f[0].left_signs == 1 && f[0].whole == 1, "reversed: %zu dense steps", f.size());

    f = dense_flags("sum", keep(gaast_expr_add(mul(in(0), in(1)), mul(in(2), in(3)))), n, euclid);
    CHECK(f.size() == 2 && f[0].beta == 0 && f[0].whole == 1 && f[1].beta == 1 && f[1].whole == 0, "sum: %zu dense steps", f.size());

    while (!handles.empty()) {
        gaast_expr_release(handles.back());
        handles.pop_back();
    }
    std::printf(g_fail ? "FAILED\n" : "ALL OK\n");
    return g_fail;
}
