// CPU-only: writes every generated artifact of every step gaast::build_plan produces for a fixed corpus -- the hiprtc sources of
// the fused-plan kernels (gaast_jit) and of the list chain (gaast_chain), the k_ast_fused micro-op stream and the tables built next
// to them -- into the directory argv[1], one file per (case, step, artifact).  tests/test_codegen_digests.py compares length and
// SHA-256 of each file with tests/golden/codegen_digests.json: the strings are what the runtime compiles and what the compiled-code
// cache is keyed by, so equal bytes mean equal results, speed and cache behaviour.  Reads only plan.hpp fields, calls only
// build_plan.  One line per step on stdout (the test checks from them that the corpus still reaches every form).
// Build: g++ -std=c++17 -O1 -I include -I gaast_amd/csrc/device -I gaast_amd/csrc/common -I gaast_amd/csrc/host
//        tests/cpp/codegen_dump_driver.cpp gaast_amd/csrc/host/{expr,c_api_host,wire}.cpp gaast_amd/csrc/device/plan*.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gaast_expr.h"
#include "plan.hpp"

static const char* g_dir = nullptr;
static int g_fail = 0;
static uint64_t full_mask(int n) { return (uint64_t(2) << n) - 1; }
static uint64_t even_mask(int n) { return 0x5555555555555555ull & full_mask(n); }
constexpr int GP = GAAST_PROD_GEOMETRIC;

static void put(const std::string& stem, const char* artifact, const void* data, size_t bytes) {
    const std::string path = std::string(g_dir) + "/" + stem + "." + artifact;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || (bytes && std::fwrite(data, 1, bytes, f) != bytes)) {
        std::fprintf(stderr, "cannot write %s\n", path.c_str());
        g_fail = 1;
    }
    if (f) std::fclose(f);
}
static void put(const std::string& stem, const char* artifact, const std::string& s) { put(stem, artifact, s.data(), s.size()); }
template <typename V>
static void put_vec(const std::string& stem, const char* artifact, const std::vector<V>& v) { put(stem, artifact, v.data(), v.size() * sizeof(V)); }

// small_reg_slab: what runtime.hip passes when it rebuilds a plan whose one-item-per-thread trial compilation used too many registers
static void dump(const char* what, gaast_expr_t e, int n, const std::vector<double>& metric, int dtype, uint32_t flags, bool small_reg_slab = false) {
    gaast_spec_t spec = gaast_expr_specialize(e, n, metric.data(), uint64_t(1) << 22);
    if (!spec) {
        std::printf("%s: specialization failed\n", what);
        g_fail = 1;
        return;
    }
    gaast_program_desc desc;
    gaast_spec_program_desc(spec, dtype, flags, &desc);
    gaast::Plan plan;
    gaast::build_plan(desc, plan, small_reg_slab);
    if (plan.steps.empty()) std::printf("%s: no steps\n", what);
    for (size_t k = 0; k < plan.steps.size(); ++k) {
        const gaast::Step& s = plan.steps[k];
        const std::string stem = std::string(what) + ".s" + std::to_string(k);
        put(stem, "name", s.name);
        std::printf("%s s%zu %s", what, k, s.name.c_str());
        if (s.kind == gaast::Step::FUSED) {
            const gaast::Step::Fused& f = s.fused;
            put(stem, "fused_jit_source", f.jit_source);
            put_vec(stem, "fused_prog", f.prog);
            put_vec(stem, "fused_phase_tab", f.phase_tab);
            put_vec(stem, "fused_general", f.general);
            std::string sc = "slab " + std::to_string(f.slab) + " out_base " + std::to_string(f.out_base) + " zero_slot " + std::to_string(f.zero_slot) +
                             " jit_threads " + std::to_string(f.jit_threads) + " jit_items " + std::to_string(f.jit_items) + " jit_persistent " +
                             std::to_string(f.jit_persistent) + " jit_only " + std::to_string(f.jit_only) + " jit_reg_trial " + std::to_string(f.jit_reg_trial) + "\n";
            for (const gaast::Step::FusedInput& fi : f.inputs) sc += "input " + std::to_string(fi.slot) + " " + std::to_string(fi.base) + " " + std::to_string(fi.canon) + "\n";
            put(stem, "fused_scalars", sc);
            std::printf(" | FUSED form=%s jit_only=%d trial=%d general=%zu", f.jit_source.empty() ? "interp" : f.jit_items ? "lds" : "reg", f.jit_only,
                        f.jit_reg_trial, f.general.size());
        }
        if (s.cj.on) {
            const gaast::Step::ChainJit& c = s.cj;
            put(stem, "cj_source", c.source);
            put_vec(stem, "cj_ent1", c.ent1);
            put_vec(stem, "cj_pos1", c.pos1);
            put_vec(stem, "cj_ent2", c.ent2);
            put_vec(stem, "cj_out2", c.out2);
            std::string sc = "single " + std::to_string(c.single) + " ipb " + std::to_string(c.ipb) + " threads " + std::to_string(c.threads) + " lds " +
                             std::to_string(c.lds) + " split " + std::to_string(c.split) + " xreg " + std::to_string(c.xreg) + "\nsorted";
            for (int v : c.sorted) sc += " " + std::to_string(v);
            sc += "\nfmt";
            for (int v : c.fmt) sc += " " + std::to_string(v);
            sc += "\nlayout";
            for (int v : c.layout) sc += " " + std::to_string(v);
            put(stem, "cj_scalars", sc + "\n");
            std::printf(" | CHAIN single=%d xreg=%d sorted=%d fmt1=%d split=%d", c.single, c.xreg, c.sorted[0] + c.sorted[1] > 0 ? 1 : 0, c.fmt[1], c.split);
        }
        std::printf("\n");
    }
    gaast_spec_free(spec);
}

static gaast_expr_t sandwich(int n, uint64_t rmask = 0) {
    gaast_expr_t r = gaast_expr_input(0, rmask ? rmask : even_mask(n), n), x = gaast_expr_input(1, 0x2, n);
    return gaast_expr_product(gaast_expr_product(r, x, GP), gaast_expr_rev(r), GP);
}
static gaast_expr_t gp(int n, uint64_t lmask, uint64_t rmask) { return gaast_expr_product(gaast_expr_input(0, lmask, n), gaast_expr_input(1, rmask, n), GP); }
static gaast_expr_t vinv(int n) { return gaast_expr_vinv(gaast_expr_input(0, even_mask(n), n)); }
static gaast_expr_t proj(int n) {   // (v & bv) & bv.vinv()
    gaast_expr_t v = gaast_expr_input(0, 0x2, n), bv = gaast_expr_input(1, 0x4, n);
    return gaast_expr_product(gaast_expr_product(v, bv, GAAST_PROD_INNER), gaast_expr_vinv(bv), GAAST_PROD_INNER);
}
static gaast_expr_t unary(int n) {   // element-wise arms, then a scaling product
    const int k = n / 2;
    gaast_expr_t a = gaast_expr_input(0, uint64_t(1) << k, n), b = gaast_expr_input(1, uint64_t(1) << k, n), sc = gaast_expr_input(2, 1, n);
    return gaast_expr_product(gaast_expr_rev(gaast_expr_add(gaast_expr_neg(gaast_expr_rev(a)), gaast_expr_ginvol(b))), sc, GP);
}
static gaast_expr_t cfg1(int n) {   // (a + b * c).g(2), full operands
    gaast_expr_t a = gaast_expr_input(0, full_mask(n), n), b = gaast_expr_input(1, full_mask(n), n), c = gaast_expr_input(2, full_mask(n), n);
    return gaast_expr_g(gaast_expr_add(a, gaast_expr_product(b, c, GP)), 2);
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s OUTPUT_DIR\n", argv[0]);
        return 2;
    }
    g_dir = argv[1];
    auto euclid = [](int n) { return std::vector<double>(size_t(n), 1.0); };
    const std::vector<double> cga{1, 1, 1, 1, -1}, stretched{2, 1, 1, 1, -1}, primes{2, 3, 5, 7, 11};
    std::vector<double> sig63 = euclid(9);
    for (int i = 6; i < 9; ++i) sig63[size_t(i)] = -1.0;
    const uint32_t NO_JIT = GAAST_FLAG_NO_JIT, NO_COALESCE = GAAST_FLAG_NO_COALESCE, LDS_12K = GAAST_FLAG_DEBUG_LDS_12K, EXACT = GAAST_FLAG_EXACT_ORDER,
                   EXP_LOG = GAAST_FLAG_EXP_LOG;

    // ---- gaast_jit, one item per lane, the slab in registers.  (Row forms as read from the dumped sources.)
    // R (16 elements): span with whole chunks in f64 and f32; X (5): span, f64 40-byte rows straddle chunks (per-element scatter), f32
    // 20-byte rows too; out (5): span, not whole.  Rows of up to 16 terms: two interpreter lines each
    dump("sandwich5_f64", sandwich(5), 5, cga, GAAST_F64, 0);
    dump("sandwich5_f32", sandwich(5), 5, cga, GAAST_F32, 0);
    dump("sandwich5_f64_nocoalesce", sandwich(5), 5, cga, GAAST_F64, NO_COALESCE);   // every row direct, 256 threads
    dump("sandwich5_f32_nocoalesce", sandwich(5), 5, cga, GAAST_F32, NO_COALESCE);
    // a metric entry 2.0: coefficients other than +-1 (hex-float literals; interpreter: LINE_MACS_GEN rows and `general`)
    dump("sandwich5_stretched_f64", sandwich(5), 5, stretched, GAAST_F64, 0);
    dump("sandwich5_stretched_f32", sandwich(5), 5, stretched, GAAST_F32, 0);
    // full R^5 product, f64: 256-byte rows are beyond the span budget, slab 97 <= 128: both inputs and the output by 128-byte lines;
    // one step of slab 97: beyond the single-step interpreter budget -> jit_only = 1
    dump("gp5_f64", gp(5, full_mask(5), full_mask(5)), 5, euclid(5), GAAST_F64, 0);
    dump("gp5_f32", gp(5, full_mask(5), full_mask(5)), 5, euclid(5), GAAST_F32, 0);          // 128-byte rows: span
    // full R^6 product: slab 193 > 128 and rows beyond the span budget: nothing goes through LDS, so the kernel is the 256-thread
    // direct form; one step beyond the interpreter budget: jit_only = 1; f64: 193 > 160, on trial
    // (EXACT_ORDER keeps the product a list, which can be fused)
    dump("gp6_f32_exact", gp(6, full_mask(6), full_mask(6)), 6, euclid(6), GAAST_F32, EXACT);
    dump("gp6_f64_exact", gp(6, full_mask(6), full_mask(6)), 6, euclid(6), GAAST_F64, EXACT);
    // full x bivector in R^5, f64: the bivector's span (5,120 bytes) leaves no room for the 9 KiB line buffer beside it: the line
    // form is dropped, the 256-byte rows are left to their lanes, the output is direct
    dump("gp5_full_bivector_f64", gp(5, full_mask(5), 0x4), 5, euclid(5), GAAST_F64, 0);
    // R^6 sandwich, f64: R (32 elements) by line, X (6) by span, the output (32: grades 1, 3, 5) by line
    dump("sandwich6_f64_exact", sandwich(6), 6, euclid(6), GAAST_F64, EXACT);
    dump("sandwich6_f32_exact", sandwich(6), 6, euclid(6), GAAST_F32, EXACT);
    // rows of 21 f64 elements (168 bytes, padded to 176): 11,264 bytes per wave -- beyond 10 KiB (no LDS at all: the direct form),
    // span (chunks straddle rows) within 12 KiB
    dump("add6_f64", gaast_expr_add(gaast_expr_input(0, 0x6, 6), gaast_expr_input(1, 0x6, 6)), 6, euclid(6), GAAST_F64, 0);
    dump("add6_f64_lds12k", gaast_expr_add(gaast_expr_input(0, 0x6, 6), gaast_expr_input(1, 0x6, 6)), 6, euclid(6), GAAST_F64, LDS_12K);
    dump("sandwich6_f64_exact_lds12k", sandwich(6), 6, euclid(6), GAAST_F64, EXACT | LDS_12K);
    {   // a + a * b: input 0 read raw (add_grades_from) and as 0.0 + x (product operand): two images
        gaast_expr_t a = gaast_expr_input(0, full_mask(3), 3), b = gaast_expr_input(1, full_mask(3), 3);
        gaast_expr_t e = gaast_expr_add(a, gaast_expr_product(a, b, GP));
        dump("a_plus_ab_f64", e, 3, euclid(3), GAAST_F64, 0);
        dump("a_plus_ab_f32", e, 3, euclid(3), GAAST_F32, 0);
        dump("a_plus_ab_f64_nojit", e, 3, euclid(3), GAAST_F64, NO_JIT);
    }
    {   // exp / log (register form or nothing): exp(B) x ~exp(B), log(exp(B)), exp of a vector (no domain-check pairs)
        gaast_expr_t b = gaast_expr_input(0, 0x4, 5), x = gaast_expr_input(1, 0x2, 5);
        gaast_expr_t r = gaast_expr_exp(b);
        gaast_expr_t sw = gaast_expr_product(gaast_expr_product(r, x, GP), gaast_expr_rev(r), GP);
        dump("exp_sandwich_f64", sw, 5, cga, GAAST_F64, EXP_LOG);
        dump("exp_sandwich_f32", sw, 5, cga, GAAST_F32, EXP_LOG);
        dump("log_exp_f64", gaast_expr_log(r), 5, cga, GAAST_F64, EXP_LOG);
        dump("log_exp_f32", gaast_expr_log(r), 5, cga, GAAST_F32, EXP_LOG);
        dump("log_rotor_f64", gaast_expr_log(gaast_expr_input(0, 0x5, 3)), 3, euclid(3), GAAST_F64, EXP_LOG);
        dump("exp_vector_f64", gaast_expr_exp(gaast_expr_input(0, 0x2, 4)), 4, euclid(4), GAAST_F64, EXP_LOG);
        dump("exp_sandwich_f64_nojit", sw, 5, cga, GAAST_F64, EXP_LOG | NO_JIT);   // no interpreter micro-ops, no JIT: not fused
    }
    // slab 171 (f64: > 160) / 259 f32 n = 8 (> 200): one item per thread ON TRIAL.  proj12: the 66-element bivector is left to its lane
    // beside the vector's span; unary8_f32 (below): 70-element operands left to their lanes, the scalar by span, output `if (false && ...)`
    dump("proj12_f64", proj(12), 12, euclid(12), GAAST_F64, 0);
    dump("vinv8_f32", vinv(8), 8, euclid(8), GAAST_F32, 0);
    dump("sinv_sqrt_f32", gaast_expr_sqrt(gaast_expr_norm_sq(gaast_expr_input(0, 0x2, 4))), 4, euclid(4), GAAST_F32, 0);   // SUNARY sqrt
    dump("sinv_sqrt_f64", gaast_expr_sqrt(gaast_expr_norm_sq(gaast_expr_input(0, 0x2, 4))), 4, euclid(4), GAAST_F64, 0);

    // ---- gaast_jit, the slabs in LDS (persistent 512-thread workgroups)
    dump("vinv8_f64", vinv(8), 8, euclid(8), GAAST_F64, 0);         // slab 259 > 256
    dump("unary8_f64", unary(8), 8, euclid(8), GAAST_F64, 0);
    dump("unary8_f32", unary(8), 8, euclid(8), GAAST_F32, 0);
    dump("vinv8_f32_small", vinv(8), 8, euclid(8), GAAST_F32, 0, true);    // the trial failed: rebuilt with small_reg_slab
    dump("proj12_f64_small", proj(12), 12, euclid(12), GAAST_F64, 0, true);
    {   // eight inputs of 33, ..., 33, 49 f64 elements: 7 * 3 + 4 = 25 > 24 16-byte pieces per thread: fast = false; slab 287
        gaast_expr_t e = gaast_expr_input(0, 0x2b, 6);
        for (int i = 1; i < 7; ++i) e = gaast_expr_add(e, gaast_expr_input(i, 0x2b, 6));
        e = gaast_expr_g(gaast_expr_add(e, gaast_expr_input(7, 0x6f, 6)), 1);
        dump("sum8_f64", e, 6, euclid(6), GAAST_F64, 0);
    }

    // ---- k_ast_fused only
    dump("sandwich5_f64_nojit", sandwich(5), 5, cga, GAAST_F64, NO_JIT);
    dump("sandwich5_stretched_f64_nojit", sandwich(5), 5, stretched, GAAST_F64, NO_JIT);   // LINE_MACS_GEN
    dump("sandwich5_stretched_f32_nojit", sandwich(5), 5, stretched, GAAST_F32, NO_JIT);
    dump("gp5_primes_f64_nojit", gp(5, full_mask(5), full_mask(5)), 5, primes, GAAST_F64, NO_JIT);   // more than six general coefficients: not fused
    dump("vinv8_f64_nojit", vinv(8), 8, euclid(8), GAAST_F64, NO_JIT);
    dump("unary8_f64_nojit", unary(8), 8, euclid(8), GAAST_F64, NO_JIT);

    // ---- gaast_chain
    for (int dtype : {GAAST_F64, GAAST_F32})
        for (uint32_t flags : {0u, EXACT}) {
            const std::string tag = std::string(dtype == GAAST_F32 ? "_f32" : "_f64") + (flags ? "_exact" : "");
            for (int n : {8, 9, 10})   // two lists: (R X ~R).g(1)
                dump(("sand" + std::to_string(n) + "g1" + tag).c_str(), gaast_expr_g(sandwich(n), 1), n, euclid(n), dtype, flags);
            dump(("sand9g1_63" + tag).c_str(), gaast_expr_g(sandwich(9), 1), 9, sig63, dtype, flags);
            for (int n : {8, 12})      // a single list, the covering copy folded in
                dump(("cfg1_" + std::to_string(n) + tag).c_str(), cfg1(n), n, euclid(n), dtype, flags);
        }
    return g_fail;
}
