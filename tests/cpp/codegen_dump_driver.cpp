// CPU-only: writes every generated artifact of every step gaast::build_plan produces for a fixed corpus -- the hiprtc sources of
// the fused-plan kernels (gaast_jit) and of the list chain (gaast_chain), the k_ast_fused micro-op stream and the tables built next
// to them, the wiring of every step, what the whole-plan passes build (plan_passes.cpp) and the plan's dead cache buffers -- into the
// directory argv[1], one file per (case, step, artifact).  tests/test_codegen_digests.py compares length and
// SHA-256 of each file with tests/golden/codegen_digests.json: the strings are what the runtime compiles and what the compiled-code
// cache is keyed by, so equal bytes mean equal results, speed and cache behaviour.  Reads only plan.hpp fields, calls only
// build_plan (and gaast_program_vjp for the adjoint programs).  One line per step on stdout (the test checks from them that the corpus still reaches every form).
// Build: g++ -std=c++17 -O1 -I include -I gaast_amd/csrc/device -I gaast_amd/csrc/common -I gaast_amd/csrc/host
//        tests/cpp/codegen_dump_driver.cpp gaast_amd/csrc/host/{expr,c_api_host,wire,vjp}.cpp gaast_amd/csrc/device/plan*.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
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

static std::string ref_text(gaast::BufRef r) { return std::to_string(int(r.kind)) + ":" + std::to_string(r.idx); }
static const char* const kFamily[] = {"VECTOR_FMA", "MFMA6", "MFMA7", "MFMA16X4", "MFMA32", "MFMA32P", "SPINOR"};

// every table and every scalar field of a product step (Step::Dense, Step::Pre under a chain, Step::List)
static void put_product(const std::string& stem, const gaast::Step& s) {
    const std::string common = "beta " + std::to_string(s.beta) + " canon_a " + std::to_string(s.canon_a) + " canon_b " + std::to_string(s.canon_b) + " a " + ref_text(s.a) +
                               " b " + ref_text(s.b) + " n_entries " + std::to_string(s.n_entries) + "\n";
    if (s.kind == gaast::Step::PRODUCT_DENSE) {
        const gaast::Step::Dense& q = s.dense;
        put_vec(stem, "dense_left_map", q.left_map);
        put_vec(stem, "dense_right_map", q.right_map);
        put_vec(stem, "dense_out_map", q.out_map);
        put_vec(stem, "dense_spinor_out_map", q.spinor_out_map);
        put_vec(stem, "dense_left_scale", q.left_scale);
        put_vec(stem, "dense_right_scale", q.right_scale);
        put_vec(stem, "dense_out_scale", q.out_scale);
        std::string sc = common + "family " + kFamily[int(q.family)] + " n " + std::to_string(q.n) + " scaled " + std::to_string(q.scaled) + " left_full " +
                         std::to_string(q.left_full) + " right_full " + std::to_string(q.right_full) + " out_full " + std::to_string(q.out_full) + " left_contig " +
                         std::to_string(q.left_contig) + " right_contig " + std::to_string(q.right_contig) + " left_signs " + std::to_string(q.left_signs) +
                         " out_signs " + std::to_string(q.out_signs) + "\nneg_hi " + std::to_string(q.neg_hi) + " zero_hi " + std::to_string(q.zero_hi) + " neg_lo " +
                         std::to_string(q.neg_lo) + " neg_lo_all " + std::to_string(q.neg_lo_all) + " degenerate " + std::to_string(q.degenerate) + " mfma16_quads " +
                         std::to_string(q.mfma16_quads) + " spinor_lam_bit " + std::to_string(q.spinor_lam_bit) + " spinor_has_alpha " +
                         std::to_string(q.spinor_has_alpha) + " spinor_m " + std::to_string(q.spinor_m) + " chained " + std::to_string(q.chained) + "\n";
        put(stem, "dense_scalars", sc);
        std::printf(" | DENSE family=%s n=%d full=%d%d contig=%d%d scaled=%d degenerate=%d neg_lo_all=%d quads=%d chained=%d row_scale=%d", kFamily[int(q.family)], q.n,
                    q.left_full, q.right_full, q.left_contig, q.right_contig, q.scaled, q.degenerate, q.neg_lo_all, q.mfma16_quads, q.chained, s.pre.row_scale.empty() ? 0 : 1);
        if (q.chained) {
            const gaast::Step::Pre& r = s.pre;
            put_vec(stem, "pre_row_start", r.row_start);
            put_vec(stem, "pre_entries", r.entries);
            put_vec(stem, "pre_coeff", r.coeff);
            put_vec(stem, "pre_row_map", r.row_map);
            put_vec(stem, "pre_row_scale", r.row_scale);
            put(stem, "pre_scalars", "a " + ref_text(r.a) + " b " + ref_text(r.b) + " canon_a " + std::to_string(r.canon_a) + " canon_b " + std::to_string(r.canon_b) +
                                         " left_len " + std::to_string(r.left_len) + " right_len " + std::to_string(r.right_len) + " width " + std::to_string(r.width) + "\n");
        }
    }
    if (s.kind == gaast::Step::PRODUCT_CSR) {
        const gaast::Step::List& q = s.list;
        put_vec(stem, "list_row_start", q.row_start);
        put_vec(stem, "list_row_out", q.row_out);
        put_vec(stem, "list_entries", q.entries);
        put_vec(stem, "list_coeff", q.coeff);
        put(stem, "list_scalars", common + "ell_width " + std::to_string(q.ell_width) + " ell_bytes " + std::to_string(q.ell_bytes) + "\n");
        size_t empty = 0;
        for (size_t r = 0; r + 1 < q.row_start.size(); ++r) empty += q.row_start[r + 1] == q.row_start[r];
        std::printf(" | LIST beta=%d rows=%zu empty_rows=%zu ell=%d", s.beta, q.row_out.size(), empty, q.ell_width);
    }
}

static std::string field(const char* name, long long v) { return std::string(" ") + name + " " + std::to_string(v); }

// how a step is wired into the plan (every kind), and every table and scalar field the whole-plan passes build (plan_passes.cpp): the
// element-wise pass, the reduction with its scaling, the list chain
static void put_pass_fields(const std::string& stem, const gaast::Step& s) {
    put(stem, "wiring", "kind " + std::to_string(int(s.kind)) + " res " + ref_text(s.res) + " a " + ref_text(s.a) + " b " + ref_text(s.b) + field("beta", s.beta) +
                            field("canon_a", s.canon_a) + field("canon_b", s.canon_b) + " pre.a " + ref_text(s.pre.a) + " pre.b " + ref_text(s.pre.b) +
                            field("n_entries", (long long)s.n_entries) + "\n");
    if (s.kind == gaast::Step::ELEMENTWISE) {
        const gaast::Step::Elementwise& q = s.ew;
        std::string src = "src";
        for (gaast::BufRef r : q.src) src += " " + ref_text(r);
        put(stem, "ew_scalars", src + "\n" + field("n_ops", q.n_ops).substr(1) + field("load_first", q.load_first) + field("scale", q.scale) + field("scalar_off", q.scalar_off) +
                                    field("canon_v", q.canon_v) + field("canon_s", q.canon_s) + field("s_is_left", q.s_is_left) + "\n");
        put_vec(stem, "ew_ops", q.ops);
        put_vec(stem, "ew_comp_off", q.comp_off);
        put_vec(stem, "ew_out_off", q.out_off);
        put_vec(stem, "ew_coeff", q.coeff);
        std::printf(" | EW scale=%d n_ops=%d", q.scale, q.n_ops);
    }
    if (s.kind == gaast::Step::REDUCE_SCALE) {
        const gaast::Step::Reduce& q = s.reduce;
        put_vec(stem, "reduce_ent1", q.ent1);
        put_vec(stem, "reduce_coeff1", q.coeff1);
        put_vec(stem, "reduce_ent2", q.ent2);
        put_vec(stem, "reduce_coeff2", q.coeff2);
        put_vec(stem, "reduce_sign_words", q.sign_words);
        put(stem, "reduce_scalars", "x " + ref_text(q.x) + field("canon_x", q.canon_x) + field("canon_s", q.canon_s) + field("s_is_left", q.s_is_left) + field("op", q.op) +
                                        field("wave", q.wave) + "\n");
        std::printf(" | REDUCE op=%d wave=%d", q.op, q.wave);
    }
    if (s.chain.side) {
        const gaast::Step::Chain& q = s.chain;
        put(stem, "chain_scalars", "side " + std::to_string(q.side) + field("alias", q.alias) + field("mid_len", q.mid_len) + field("canon_mid", q.canon_mid) +
                                       field("covered", q.covered) + field("ipb", q.ipb) + field("item_stride", q.item_stride) + field("ent2_lds", q.ent2_lds) + "\n");
        std::printf(" | LINK side=%d alias=%d", q.side, q.alias);
    }
}

// small_reg_slab: what runtime.hip passes when it rebuilds a plan whose one-item-per-thread trial compilation used too many registers;
// mirrored: the orthogonal basis of a Gram metric whose Q has det -1
static void dump_desc(const char* what, const gaast_program_desc& desc, bool small_reg_slab = false, bool mirrored = false) {
    gaast::Plan plan;
    gaast::build_plan(desc, plan, small_reg_slab, mirrored);
    if (plan.steps.empty()) std::printf("%s: no steps\n", what);
    {   // the cache buffers no launch needs
        std::string dead = "node_buffers " + std::to_string(plan.node_buffers.size()) + " node_dead";
        for (char c : plan.node_dead) dead += c ? " 1" : " 0";
        put(what, "plan_node_dead", dead + "\n");
    }
    for (size_t k = 0; k < plan.steps.size(); ++k) {
        const gaast::Step& s = plan.steps[k];
        const std::string stem = std::string(what) + ".s" + std::to_string(k);
        put(stem, "name", s.name);
        std::printf("%s s%zu %s", what, k, s.name.c_str());
        put_product(stem, s);
        put_pass_fields(stem, s);
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
}

static void dump(const char* what, gaast_expr_t e, int n, const std::vector<double>& metric, int dtype, uint32_t flags, bool small_reg_slab = false, bool mirrored = false) {
    gaast_spec_t spec = gaast_expr_specialize(e, n, metric.data(), uint64_t(1) << 22);
    if (!spec) {
        std::printf("%s: specialization failed: %s\n", what, gaast_expr_last_error());
        g_fail = 1;
        return;
    }
    gaast_program_desc desc;
    gaast_spec_program_desc(spec, dtype, flags, &desc);
    dump_desc(what, desc, small_reg_slab, mirrored);
    gaast_spec_free(spec);
}

// the reverse-mode program of `e` with respect to input `wrt` (gaast_program_vjp): adjoint product nodes
static void dump_vjp(const char* what, gaast_expr_t e, int n, const std::vector<double>& metric, int dtype, uint32_t flags, int wrt) {
    gaast_spec_t spec = gaast_expr_specialize(e, n, metric.data(), uint64_t(1) << 22);
    gaast_program_desc desc;
    gaast_program_image_t img = nullptr;
    if (!spec || gaast_spec_program_desc(spec, dtype, flags, &desc) != 0 || gaast_program_vjp(&desc, wrt, &img) != 0 || !img) {
        std::printf("%s: no reverse-mode program\n", what);
        g_fail = 1;
    } else {
        dump_desc(what, *gaast_program_image_desc(img));
        gaast_program_image_free(img);
    }
    if (spec) gaast_spec_free(spec);
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
static gaast_expr_t unary_unscaled(int n) {   // ... without the scaling product
    const int k = n / 2;
    gaast_expr_t a = gaast_expr_input(0, uint64_t(1) << k, n), b = gaast_expr_input(1, uint64_t(1) << k, n);
    return gaast_expr_rev(gaast_expr_add(gaast_expr_neg(gaast_expr_rev(a)), gaast_expr_ginvol(b)));
}
static gaast_expr_t times_norm(int n, bool root) {   // a * norm_sq(a) / a * sqrt(norm_sq(a)), a even
    gaast_expr_t a = gaast_expr_input(0, even_mask(n), n), s = gaast_expr_norm_sq(a);
    return gaast_expr_product(a, root ? gaast_expr_sqrt(s) : s, GP);
}
static gaast_expr_t sandwich_right_first(int n) {   // R (X ~R): the mid row is the second list's RIGHT operand
    gaast_expr_t r = gaast_expr_input(0, even_mask(n), n), x = gaast_expr_input(1, 0x2, n);
    return gaast_expr_product(r, gaast_expr_product(x, gaast_expr_rev(r), GP), GP);
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

    // ---- the product lowering: every dense kernel family and every branch of its operand images, the matrix-representation tables,
    // chained products and the exact list (tests/test_codegen_digests.py: test_corpus_reaches_every_branch_of_the_product_lowering)
    const uint32_t NO_MFMA = GAAST_FLAG_NO_MFMA, SPINOR = GAAST_FLAG_SPINOR_GEMM;
    auto with = [&](int n, std::initializer_list<std::pair<int, double>> entries) {
        std::vector<double> m = euclid(n);
        for (const auto& e : entries) m[size_t(e.first)] = e.second;
        return m;
    };
    auto full = [](int n) { return gp(n, full_mask(n), full_mask(n)); };
    const uint64_t odd8 = full_mask(8) & ~even_mask(8);
    const std::vector<double> primes8{2, 3, 5, 7, 11, 13, 17, 19}, null8 = with(8, {{7, 0.0}});
    for (int dtype : {GAAST_F32, GAAST_F64}) {
        const std::string t = dtype == GAAST_F32 ? "_f32" : "_f64";
        dump(("dense_vf8" + t).c_str(), full(8), 8, euclid(8), dtype, NO_MFMA);                          // VECTOR_FMA
        dump(("dense_gp6" + t).c_str(), full(6), 6, euclid(6), dtype, 0);                                // MFMA6, entries dealt to lanes
        dump(("dense_gp6_partial" + t).c_str(), gp(6, full_mask(6), even_mask(6)), 6, euclid(6), dtype, 0);
        dump(("dense_gp7" + t).c_str(), full(7), 7, euclid(7), dtype, 0);                                // MFMA7, entries dealt by bank
        dump(("dense_gp7_partial" + t).c_str(), gp(7, full_mask(7), even_mask(7)), 7, euclid(7), dtype, 0);
        dump(("dense_gp8" + t).c_str(), full(8), 8, euclid(8), dtype, 0);                                // MFMA16X4: f64 B image / f32 quad image
        dump(("dense_gp8_null" + t).c_str(), full(8), 8, null8, dtype, 0);
        for (int n : {8, 9})                                                                              // R X ~R: the list R X in the dense kernel's LDS
            dump(("dense_sandwich" + std::to_string(n) + t).c_str(), sandwich(n), n, euclid(n), dtype, 0);
    }
    dump("dense_sandwich8_primes_f32", sandwich(8), 8, primes8, GAAST_F32, 0);                            // ... on a rescaled basis: row_scale
    dump("dense_vf8_neglo_f32", full(8), 8, with(8, {{0, -1.0}, {1, -1.0}, {2, -1.0}, {3, -1.0}, {7, -1.0}}), GAAST_F32, NO_MFMA);   // all four lo vectors negative
    dump("dense_vf8_permuted_f32", full(8), 8, with(8, {{0, -1.0}}), GAAST_F32, NO_MFMA);               // the identity basis does not qualify
    dump("dense_gp10_f32", full(10), 10, euclid(10), GAAST_F32, 0);                                      // MFMA32P, block image
    dump("dense_gp12_f32", full(12), 12, euclid(12), GAAST_F32, 0);                                      // ... quad-plane image
    dump("dense_gp12_null_f32", full(12), 12, with(12, {{11, 0.0}}), GAAST_F32, 0);                      // ... a null hi vector: block image, degenerate
    dump("dense_gp14_f32", full(14), 14, euclid(14), GAAST_F32, 0);                                      // MFMA32
    dump("dense_ee8_f32", gp(8, even_mask(8), even_mask(8)), 8, euclid(8), GAAST_F32, 0);                // parity-pure operands: one product in Cl(7)
    dump("dense_oe8_f32", gp(8, odd8, even_mask(8)), 8, euclid(8), GAAST_F32, 0);
    dump("dense_eo8_f32", gp(8, even_mask(8), odd8), 8, euclid(8), GAAST_F32, 0);
    dump("dense_oo8_f32", gp(8, odd8, odd8), 8, euclid(8), GAAST_F32, 0);
    dump("dense_oe8_pivot2_f32", gp(8, odd8, even_mask(8)), 8, with(8, {{7, 2.0}}), GAAST_F32, 0);       // a pivot that squares to 2
    dump("dense_oo8_pivot2_f64", gp(8, odd8, odd8), 8, with(8, {{7, 2.0}}), GAAST_F64, 0);
    dump("dense_gp8_primes_f32", full(8), 8, primes8, GAAST_F32, 0);                                     // rescaled basis
    dump("dense_gp8_primes_f64", full(8), 8, primes8, GAAST_F64, 0);
    dump("dense_gp8_negfirst_f32", full(8), 8, with(8, {{0, -1.0}, {1, -1.0}}), GAAST_F32, 0);           // negative vectors first
    for (int wrt : {0, 1}) {                                                                              // adjoints of a geometric product
        const std::string w = wrt ? "_right" : "_left";
        dump_vjp(("dense_adj8" + w + "_f32").c_str(), full(8), 8, euclid(8), GAAST_F32, 0, wrt);
        dump_vjp(("dense_adj8_null" + w + "_f32").c_str(), full(8), 8, null8, GAAST_F32, 0, wrt);
        dump_vjp(("dense_adj8_primes" + w + "_f64").c_str(), full(8), 8, primes8, GAAST_F64, 0, wrt);
    }
    dump("spinor8_f32", full(8), 8, euclid(8), GAAST_F32, SPINOR);
    dump("spinor7_f32", full(7), 7, euclid(7), GAAST_F32, SPINOR);                                        // padded to n + 1
    dump("spinor8_neg_f32", full(8), 8, with(8, {{2, -1.0}}), GAAST_F32, SPINOR);
    {   // the exact list: a fresh result; one whose buffer holds a grade only the NEXT arm fills (rows nothing is added to; an accumulated
        // list: cfg1_* above); the orientation sign of a mirrored Gram basis on a regressive list; a compact adjoint no dense kernel takes
        gaast_expr_t a = gaast_expr_input(0, 0x4, 12), b = gaast_expr_input(1, full_mask(12), 12), c = gaast_expr_input(2, full_mask(11), 12);
        dump("list_fresh12_null_f64", gaast_expr_product(a, b, GAAST_PROD_INNER), 12, with(12, {{11, 0.0}}), GAAST_F64, 0);
        dump("list_fresh12_empty_rows_f32", gaast_expr_add(gaast_expr_product(a, b, GAAST_PROD_INNER), c), 12, euclid(12), GAAST_F32, 0);
        dump("list_regressive12_mirrored_f64", gaast_expr_product(b, gaast_expr_input(3, uint64_t(3) << 10, 12), GAAST_PROD_REGRESSIVE), 12, euclid(12), GAAST_F64, 0, false, true);
        dump_vjp("list_adj8_exact_f32", full(8), 8, euclid(8), GAAST_F32, EXACT, 0);
    }

    // ---- the whole-plan passes the cases above do not reach (tests/test_codegen_digests.py: test_corpus_reaches_every_form_of_the_plan_passes)
    for (int dtype : {GAAST_F32, GAAST_F64}) {
        const std::string t = dtype == GAAST_F32 ? "_f32" : "_f64";
        // five element-wise arms on grade-6 rows in one pass; with the scaling product as its epilogue: the run's buffer is dead
        dump(("unary12" + t).c_str(), unary(12), 12, euclid(12), dtype, 0);
        dump(("unary12_unscaled" + t).c_str(), unary_unscaled(12), 12, euclid(12), dtype, 0);
        for (int n : {10, 12})   // reduce_scale, 1 / s: a wave keeps the row in registers (tolerance mode) / streams it (exact order)
            for (uint32_t flags : {0u, EXACT})
                dump(("vinv" + std::to_string(n) + t + (flags ? "_exact" : "")).c_str(), vinv(n), n, euclid(n), dtype, flags);
    }
    dump("times_sqrt_norm12_f64", times_norm(12, true), 12, euclid(12), GAAST_F64, 0);    // reduce_scale, sqrt(s)
    dump("times_norm12_f64", times_norm(12, false), 12, euclid(12), GAAST_F64, 0);        // reduce_scale, the scalar as it is
    dump("sand9g1_right_first_f64", gaast_expr_g(sandwich_right_first(9), 1), 9, euclid(9), GAAST_F64, 0);   // list chain, side 2
    return g_fail;
}
