// Whole-plan fusion for small programs: every buffer becomes a region of a per-item slab and the steps become ONE launch -- the
// k_ast_fused micro-op stream, and the same plan as straight-line HIP specialised through hiprtc (gaast_jit), with the slab in
// registers (one item per lane) or the slabs in LDS (persistent 512-thread workgroups).  Exact: same operations, same order.
// The generated text is pinned byte for byte by tests/test_codegen_digests.py.
#include "plan_internal.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>

#ifndef GAAST_JIT_NT
#define GAAST_JIT_NT 3   /* bit 0: nontemporal span stores, bit 1: nontemporal span loads in the specialised kernels (A/B switch; both: config 5 0.70 -> 0.78-0.82 of 8 TB/s) */
#endif
namespace gaast {
namespace {

std::string str(long long v) { return std::to_string(v); }

// ---------------------------------------------------------------------------------------------
// Where every buffer of the plan lives in the per-item slab, and which kernels may run it.
// ---------------------------------------------------------------------------------------------
struct SlabLayout {
    const Plan& plan;
    bool ok = false;   // the plan can be fused
    // an input read both ways gets two images: the raw rows (add_grades_from) and 0.0 + x
    // (the zero-init + copy the reference makes of a product operand)
    std::vector<int> in_base, in_base_canon, node_base;
    std::vector<Step::FusedInput> inputs;
    int out_base = 0;
    int zero_slot = 0;   // one element per item holding +0.0: target of unused MAC slots
    int slab = 0;        // odd: 64 lanes at one slab offset hit 64 different banks
    size_t elem = 8;
    bool interp_ok = false, jit_allowed = false;
    int jit_slab_small = 0;

    SlabLayout(const Plan& p, bool small_reg_slab);
    int base_of(BufRef r, int canon = 0) const {
        return r.kind == BufKind::NODE    ? node_base[size_t(r.idx)]
               : r.kind == BufKind::INPUT ? (canon ? in_base_canon : in_base)[size_t(r.idx)]
                                          : out_base;
    }
    int input_len(size_t i) const { return int(plan.input_layouts[size_t(inputs[i].slot)].row_len); }
};

SlabLayout::SlabLayout(const Plan& p, bool small_reg_slab) : plan(p), elem(p.dtype == GAAST_F32 ? 4 : 8) {
    if (plan.flags & GAAST_FLAG_NO_FUSION) return;
    if (plan.error != GAAST_OK || plan.steps.empty()) return;
    // which buffers are touched, and how inputs are read
    std::vector<int> in_direct(plan.inputs.size(), 0), in_axpy(plan.inputs.size(), 0);
    for (const Step& s : plan.steps) {
        if (s.kind == Step::PRODUCT_DENSE || s.kind == Step::FUSED || s.kind == Step::INVERSE || s.kind == Step::GEXP || s.kind == Step::GEXP_ADJ || s.kind == Step::GSQRT || s.kind == Step::GSQRT_ADJ || s.kind == Step::GLOG || s.kind == Step::GLOG_ADJ || s.kind == Step::GEXP_JVP || s.kind == Step::GEXP_ADJ2 || s.kind == Step::GSQRT_JVP || s.kind == Step::GLOG_JVP || s.kind == Step::GLOG_ADJ2) return;   // (an inverse, a general exponential, a general square root, a general logarithm, their adjoints, the second-order steps of exponential and logarithm and the tangents of root and logarithm are always launches of their own)
        if (s.kind == Step::AXPY) in_axpy[size_t(s.a.idx)] = 1;
        if (s.kind == Step::DUAL && s.a.kind == BufKind::INPUT) (s.canon_a ? in_direct : in_axpy)[size_t(s.a.idx)] = 1;
        if (s.kind == Step::PRODUCT_CSR) {
            if (s.a.kind == BufKind::INPUT) (s.canon_a ? in_direct : in_axpy)[size_t(s.a.idx)] = 1;
            if (s.b.kind == BufKind::INPUT) (s.canon_b ? in_direct : in_axpy)[size_t(s.b.idx)] = 1;
        }
    }
    int cursor = 0;
    in_base.assign(plan.inputs.size(), -1);
    in_base_canon.assign(plan.inputs.size(), -1);
    node_base.assign(plan.node_buffers.size(), -1);
    for (size_t i = 0; i < plan.inputs.size(); ++i) {
        if (plan.input_layouts[i].row_len == 0) continue;
        if (in_axpy[i]) {
            in_base[i] = cursor;
            inputs.push_back({int(i), cursor, 0});
            cursor += int(plan.input_layouts[i].row_len);
        }
        if (in_direct[i]) {
            in_base_canon[i] = cursor;
            inputs.push_back({int(i), cursor, 1});
            cursor += int(plan.input_layouts[i].row_len);
        }
    }
    if (inputs.size() > size_t(uop::MAX_INPUTS)) return;
    for (size_t i = 0; i < plan.node_buffers.size(); ++i) {
        node_base[i] = cursor;
        cursor += int(plan.node_buffers[i].row_len);
    }
    out_base = cursor;
    cursor += int(plan.out_layout.row_len);
    if (plan.out_layout.row_len == 0) return;
    zero_slot = cursor++;
    slab = cursor | 1;
    // the LDS interpreter kernel needs the slabs of 64 items in 48 KiB; the hiprtc-specialised kernel keeps the slab
    // in registers and only needs it to be small enough for that -- plans that fit only the latter are fused
    // "JIT only" (the runtime falls back to an unfused plan if the compilation fails)
    // (plans with exp / log steps or their adjoints have no interpreter micro-ops: the specialised kernel or nothing)
    // (round 3: 144 KiB instead of 48 -- one 512-thread workgroup per CU -- so that programs whose slab is beyond the registers of
    //  the specialised kernel but whose lists are short still run as ONE launch: the projected sandwich (R X ~R).g(1) at n = 7, 8
    //  has two lists of n 2^(n-1) entries over a slab of 2^n + 2 n elements; as two list launches it ran 8 active lanes per item)
    //  -- for plans of SEVERAL steps only: a single big list is better off on k_product_ell (twice the terms per second)
    const size_t interp_budget = plan.steps.size() >= 2 ? kInterpLdsBytes : size_t(48 * 1024);
    interp_ok = !(slab > 4095 || size_t(slab) * elem > 32767 || size_t(slab) * elem * 64 > interp_budget) && !plan.has_explog && !plan.has_explog_adj;
    // One item per thread, the slab in registers: up to 160 (f64) / 200 (f32) elements always; up to 256 / 320 ON TRIAL -- the
    // compiler keeps only the LIVE values in registers, the projection (v & bv) & bv.vinv() at n = 12 (slab 171) compiles to 222
    // registers and runs at 0.75 of the HBM roof against 0.44 with its slabs in LDS, the versor inverse at n = 8 (slab 259: the
    // whole row is live until it is scaled) to 310 with one wave per SIMD and 0.46 against 0.67.  The runtime measures the compiled
    // kernel's occupancy and rebuilds the plan with small_reg_slab when the trial fails.
    jit_slab_small = plan.dtype == GAAST_F32 ? 200 : 160;
    const int jit_slab_limit = small_reg_slab ? jit_slab_small : (plan.dtype == GAAST_F32 ? 320 : 256);
    jit_allowed = !(plan.flags & GAAST_FLAG_NO_JIT) && slab <= jit_slab_limit;
    ok = interp_ok || jit_allowed;
}

// Independent pieces of a step are dealt to the eight waves of a workgroup, least-loaded first (k_ast_fused and the slabs-in-LDS form
// of gaast_jit share the schedule).  Any split is exact: rows of one Product never read what another row of the same Product writes.
struct WaveLoads {
    uint64_t load[uop::GROUPS] = {};
    int take(uint64_t cost) {   // the wave that gets a piece of this cost
        int g = 0;
        for (int i = 1; i < uop::GROUPS; ++i)
            if (load[i] < load[g]) g = i;
        load[g] += cost;
        return g;
    }
};

// ---------------------------------------------------------------------------------------------
// The plan as the k_ast_fused micro-op stream: one phase per step (fused.prog, phase_tab, general; see kernels.hip.hpp).
// false: a step or a coefficient set the interpreter has no encoding for.  entries: the comp-muls encoded.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t LW = 32;   // words per line

// one result row of a list: lines of up to 10 terms
bool encode_row(const Step& s, size_t row, uint32_t rb, uint32_t lb, uint32_t rrb, uint32_t esz, std::vector<double>& general, std::vector<uint32_t>& out) {
    const uint32_t dst = rb + s.list.row_out[row];
    const uint32_t e0 = s.list.row_start[row], e1 = s.list.row_start[row + 1];
    bool row_general = false;
    for (uint32_t e = e0; e < e1; ++e) row_general |= (s.list.coeff[e] != 1.0 && s.list.coeff[e] != -1.0);
    // split long rows evenly over their lines (16 entries -> 8 + 8, not 10 + 6)
    const uint32_t n_l = e1 > e0 ? (e1 - e0 + 9) / 10 : 1;
    const uint32_t per = e1 > e0 ? (e1 - e0 + n_l - 1) / n_l : 0;
    uint32_t e = e0;
    do {  // a row with no entries still stores its (fresh) 0.0
        const uint32_t cnt = std::min<uint32_t>(per, e1 - e);
        uint32_t hdr = dst | (cnt << 15);
        if (e == e0) hdr |= (1u << 12) | (s.beta ? 0u : (1u << 13));
        if (e + cnt == e1) hdr |= 1u << 14;
        hdr |= uint32_t(row_general ? uop::LINE_MACS_GEN : uop::LINE_MACS) << 28;
        const size_t line0 = out.size();
        out.resize(line0 + LW, 0u);
        out[line0] = hdr;
        for (uint32_t k = 0; k < cnt; ++k) {
            const double c = s.list.coeff[e + k];
            const uint32_t lo = lb + (s.list.entries[e + k] & 0xffffu), ro = rrb + (s.list.entries[e + k] >> 16);
            if (!row_general) {
                out[line0 + 2 + 3 * k] = lo * esz;
                out[line0 + 3 + 3 * k] = ro * esz;
                out[line0 + 4 + 3 * k] = c == -1.0 ? 0x80000000u : 0u;
                continue;
            }
            uint32_t ci = c == 1.0 ? 0 : 1;
            if (c != 1.0 && c != -1.0) {
                size_t gi = 0;
                for (; gi < general.size(); ++gi)
                    if (std::memcmp(&general[gi], &c, sizeof(double)) == 0) break;
                if (gi == general.size()) {
                    if (general.size() == size_t(uop::MAX_GENERAL_COEFFS)) return false;
                    general.push_back(c);
                }
                ci = uint32_t(gi) + 2;
            }
            out[line0 + 2 + 3 * k] = lo | (ro << 12);
            out[line0 + 3 + 3 * k] = ci;
        }
        e += cnt;
    } while (e < e1);
    return true;
}

bool encode_uops(const SlabLayout& lay, Step::Fused& f, uint64_t& entries) {
    constexpr int G = uop::GROUPS;
    auto mop = [](uint32_t code, uint32_t lo, uint32_t mid = 0) { return (code << 28) | (mid << 12) | lo; };
    for (const Step& s : lay.plan.steps) {
        std::vector<std::vector<uint32_t>> glines(G);  // lines of each wave, this phase
        WaveLoads waves;
        const uint32_t rb = uint32_t(lay.base_of(s.res));
        std::vector<uint32_t> misc;   // element-wise ops: chunks of <= 30, dealt round
        switch (s.kind) {
        case Step::ZERO: {
            const uint32_t len = uint32_t(lay.plan.layout(s.res).row_len);
            for (uint32_t o = 0; o < len; o += 8) misc.push_back(mop(uop::ZERO, rb + o, std::min<uint32_t>(8, len - o)));
            break;
        }
        case Step::AXPY:
            for (uint32_t m : s.axpy_map) misc.push_back(mop(s.beta ? uop::ADD : uop::COPY, rb + (m & 0xffffu), uint32_t(lay.base_of(s.a)) + (m >> 16)));   // (COPY: the zero fill folded in)
            break;
        case Step::FLIP:
            for (uint32_t o : s.flip_offsets) misc.push_back(mop(uop::NEG, rb + o));
            break;
        case Step::SUNARY:
            misc.push_back(mop(s.sunary_op == 0 ? uop::INV : uop::SQRT, rb + uint32_t(s.sunary_off)));
            break;
        case Step::PRODUCT_CSR: {
            const uint32_t lb = uint32_t(lay.base_of(s.a, s.canon_a)), rrb = uint32_t(lay.base_of(s.b, s.canon_b));
            for (size_t row = 0; row + 1 < s.list.row_start.size(); ++row) {
                const uint32_t terms = s.list.row_start[row + 1] - s.list.row_start[row];
                if (!encode_row(s, row, rb, lb, rrb, uint32_t(lay.elem), f.general, glines[size_t(waves.take(terms + 2))])) return false;
                entries += terms;
            }
            break;
        }
        case Step::EXPLOG: break;   // specialised kernel only (interp_ok is false)
        case Step::EXPLOG_ADJ: break;
        case Step::DUAL: {
            const uint32_t ab = uint32_t(lay.base_of(s.a, s.canon_a));
            s.dual.for_each([&](uint32_t r, uint32_t a, bool neg) {
                misc.push_back(mop(s.beta ? (neg ? uop::SUB : uop::ADD) : (neg ? uop::NCOPY : uop::COPY), rb + r, ab + a));
            });
            break;
        }
        default: return false;
        }
        const size_t per = std::max<size_t>(1, std::min<size_t>(30, (misc.size() + G - 1) / G));
        for (size_t i = 0; i < misc.size(); i += per) {
            const size_t cnt = std::min(per, misc.size() - i);
            std::vector<uint32_t>& out = glines[size_t(waves.take(cnt))];
            out.push_back((uint32_t(uop::LINE_MISC) << 28) | (uint32_t(cnt) << 15));
            out.push_back(0u);
            for (size_t k = 0; k < 30; ++k) out.push_back(k < cnt ? misc[i + k] : 0u);
        }
        for (int g = 0; g < G; ++g) {
            f.phase_tab.push_back(uint32_t(f.prog.size() / LW));
            f.phase_tab.push_back(uint32_t(glines[size_t(g)].size() / LW));
            f.prog.insert(f.prog.end(), glines[size_t(g)].begin(), glines[size_t(g)].end());
        }
    }
    if (f.prog.size() > (1u << 20)) return false;
    if (f.prog.empty()) f.prog.assign(LW, uint32_t(uop::LINE_NOP) << 28);
    return true;
}

// ---------------------------------------------------------------------------------------------
// The same plan as straight-line HIP source, specialised at program_create through hiprtc (the reference's README lists code
// generation from the specialized AST as roadmap).  lane <-> item, offsets and signs are constants, the statements are the
// reference's in the reference's order; the runtime compiles it with -ffp-contract=off so that the roundings stay those of eval.rs:82.
// ---------------------------------------------------------------------------------------------
struct CodeText {   // what both forms of gaast_jit spell the same way
    bool f32;
    const char* ty() const { return f32 ? "float" : "double"; }
    std::string lit(double c) const {
        char buf[256];
        std::snprintf(buf, sizeof(buf), f32 ? "%af" : "%a", f32 ? double(float(c)) : c);
        return std::string(buf);
    }
    std::string fn(const char* name) const { return std::string(name) + (f32 ? "f" : ""); }
    // the kernel's parameters up to `batch`
    std::string signature(size_t n_inputs) const {
        std::string s;
        for (size_t i = 0; i < n_inputs; ++i) s += "const T* __restrict__ in" + str(i) + ", long long s" + str(i) + ", ";
        return s + "T* __restrict__ out, long long so, long long batch";
    }
};

// How a form of the kernel writes a step's statements: the name of slab element i (`v12`: a register, `my[12]`: the item's slab in
// LDS), the indentation of a statement, how many element-wise statements make one piece.
struct StmtStyle {
    std::function<std::string(uint32_t)> el;
    std::string indent;
    size_t chunk;
};
using StmtSink = std::function<void(uint64_t cost, const std::string& text)>;   // an independent piece of the step

// exp / log: the statements of oracle/gaast_oracle.c: ext_exp_log, in its order
std::string explog_statements(const SlabLayout& lay, const Step& s, const StmtStyle& st, const CodeText& ct) {
    const uint32_t rb = uint32_t(lay.base_of(s.res)), ab = uint32_t(lay.base_of(s.a));
    const std::string in1 = st.indent, in2 = in1 + "  ", in3 = in2 + "  ";
    auto B = [&](uint32_t i) { return st.el(ab + uint32_t(s.explog.arg_k) + i); };
    std::string src = in1 + "{ T sq = T(0), nrm = T(0), viol = T(0);\n";
    for (int i = 0; i < s.explog.m; ++i) {
        src += in2 + "sq = sq + " + B(uint32_t(i)) + " * " + B(uint32_t(i)) + " * T(" + ct.lit(s.explog.sq[size_t(i)]) + ");\n";
        src += in2 + "nrm = nrm + " + B(uint32_t(i)) + " * " + B(uint32_t(i)) + ";\n";
    }
    for (size_t row = 0; row + 1 < s.explog.row_start.size(); ++row) {
        src += in2 + "{ T acc = T(0);\n";
        for (uint32_t e = s.explog.row_start[row]; e < s.explog.row_start[row + 1]; ++e)
            src += in3 + "acc = acc + " + B(s.explog.pairs[e] & 0xffffu) + " * " + B(s.explog.pairs[e] >> 16) + " * T(" + ct.lit(s.explog.pair_coeff[e]) + ");\n";
        src += in3 + "viol = viol + acc * acc; }\n";
    }
    if (s.explog.row_start.size() > 1) src += in2 + "if (viol > T(" + ct.lit(9.094947017729282e-13) + ") * (nrm * nrm)) atomicAdd(dom, 1ull);\n";
    src += in2 + "T c0 = T(0), f;\n";
    if (s.explog.op == 0) {
        src += in2 + "if (sq < T(0)) { const T t = " + ct.fn("sqrt") + "(-sq); c0 = " + ct.fn("cos") + "(t); f = " + ct.fn("sin") + "(t) / t; }\n";
        src += in2 + "else if (sq > T(0)) { const T t = " + ct.fn("sqrt") + "(sq); c0 = " + ct.fn("cosh") + "(t); f = " + ct.fn("sinh") + "(t) / t; }\n";
        src += in2 + "else if (sq == T(0)) { c0 = T(1); f = T(1); }\n" + in2 + "else { c0 = sq; f = sq; }\n";
    } else {
        const std::string a = s.explog.arg_0 >= 0 ? st.el(ab + uint32_t(s.explog.arg_0)) : std::string("T(0)");
        src += in2 + "if (sq < T(0)) { const T mm = " + ct.fn("sqrt") + "(-sq); f = " + ct.fn("atan2") + "(mm, " + a + ") / mm; }\n";
        src += in2 + "else if (sq > T(0)) { const T mm = " + ct.fn("sqrt") + "(sq); f = " + ct.fn("atanh") + "(mm / " + a + ") / mm; }\n";
        src += in2 + "else if (sq == T(0)) { f = T(1) / " + a + "; }\n" + in2 + "else { f = sq; }\n";
    }
    if (s.explog.res_0 >= 0) {
        const std::string d = st.el(rb + uint32_t(s.explog.res_0));
        src += in2 + d + " = " + d + " + c0;\n";
    }
    if (s.explog.res_k >= 0)
        for (int i = 0; i < s.explog.mres; ++i) {
            const std::string d = st.el(rb + uint32_t(s.explog.res_k) + uint32_t(i));
            src += in2 + d + " = " + d + " + f * " + B(uint32_t(i)) + ";\n";
        }
    return src + in1 + "}\n";
}

// exp / log adjoint (gaast_hip.h: GAAST_OP_EXP_ADJ / GAAST_OP_LOG_ADJ): the statements of k_exp_log_adj, in its order
std::string explog_adj_statements(const SlabLayout& lay, const Step& s, const StmtStyle& st, const CodeText& ct) {
    const Step::ExpLogAdj& q = s.adj;
    const uint32_t rb = uint32_t(lay.base_of(s.res)), ab = uint32_t(lay.base_of(s.a)), gb = uint32_t(lay.base_of(s.b));
    const std::string in1 = st.indent, in2 = in1 + "  ", in3 = in2 + "  ";
    auto B = [&](int i) { return st.el(ab + uint32_t(q.arg_k) + uint32_t(i)); };
    auto G = [&](int i) { return st.el(gb + uint32_t(q.g_k) + uint32_t(i)); };
    auto horner = [&](const std::string& x, int terms, double (*coeff)(int)) {
        std::string t = in3 + "h = T(" + ct.lit(coeff(terms)) + ");\n";
        for (int n = terms - 1; n >= 1; --n) t += in3 + "h = h * " + x + " + T(" + ct.lit(coeff(n)) + ");\n";
        return t;
    };
    std::string src = in1 + "{ T sq = T(0), dd = T(0);\n";
    for (int i = 0; i < q.m; ++i) src += in2 + "sq = sq + " + B(i) + " * " + B(i) + " * T(" + ct.lit(q.sq[size_t(i)]) + ");\n";
    for (int i = 0; i < q.mg; ++i) src += in2 + "dd = dd + " + G(i) + " * " + B(i) + ";\n";
    src += in2 + (q.op == 0 ? "T c0 = T(0), f, h, w;\n" : "T f, h, w;\n");
    if (q.op == 0) {
        src += in2 + "if (sq < T(0)) { const T t = " + ct.fn("sqrt") + "(-sq); c0 = " + ct.fn("cos") + "(t); f = " + ct.fn("sin") + "(t) / t; }\n";
        src += in2 + "else if (sq > T(0)) { const T t = " + ct.fn("sqrt") + "(sq); c0 = " + ct.fn("cosh") + "(t); f = " + ct.fn("sinh") + "(t) / t; }\n";
        src += in2 + "else if (sq == T(0)) { c0 = T(1); f = T(1); }\n" + in2 + "else { c0 = sq; f = sq; }\n";
        src += in2 + "if (sq < T(" + ct.lit(kExpAdjSeriesBelow) + ") && sq > T(" + ct.lit(-kExpAdjSeriesBelow) + ")) {\n" +
               horner("sq", exp_adj_series_terms(ct.f32), exp_adj_series_coeff) + in2 + "} else h = (c0 - f) / sq;\n";
        src += in2 + "w = f * " + (q.g_0 >= 0 ? st.el(gb + uint32_t(q.g_0)) : std::string("T(0)")) + " + h * dd;\n";
    } else {
        const std::string a = q.arg_0 >= 0 ? st.el(ab + uint32_t(q.arg_0)) : std::string("T(0)");
        src += in2 + "const T a = " + a + ";\n";
        src += in2 + "if (sq < T(0)) { const T mm = " + ct.fn("sqrt") + "(-sq); f = " + ct.fn("atan2") + "(mm, a) / mm; }\n";
        src += in2 + "else if (sq > T(0)) { const T mm = " + ct.fn("sqrt") + "(sq); f = " + ct.fn("atanh") + "(mm / a) / mm; }\n";
        src += in2 + "else if (sq == T(0)) { f = T(1) / a; }\n" + in2 + "else { f = sq; }\n";
        src += in2 + "const T a2 = a * a, D = a2 - sq, lim = T(" + ct.lit(kLogAdjSeriesBelow) + ") * a2;\n";
        src += in2 + "if (sq == T(0) || (sq < lim && sq > -lim && (a > T(0) || sq > T(0)))) {\n" + in3 + "const T u = sq / a2;\n" +
               horner("u", log_adj_series_terms(ct.f32), log_adj_series_coeff) + in3 + "h = h / (a2 * a);\n" + in2 + "} else h = (a / D - f) / sq;\n";
        src += in2 + "w = h * dd;\n";
    }
    if (q.res_k >= 0)
        for (int i = 0; i < q.mres; ++i) {
            const std::string d = st.el(rb + uint32_t(q.res_k) + uint32_t(i));
            const std::string second = "T(" + ct.lit(q.sq[size_t(i)]) + ") * " + B(i) + " * w";
            src += in2 + d + " = " + d + " + (" + (i < q.mg ? "f * " + G(i) + " + " : std::string()) + second + ");\n";
        }
    if (q.op == 1 && q.res_0 >= 0) {
        const std::string d = st.el(rb + uint32_t(q.res_0));
        src += in2 + d + " = " + d + " + (-(dd / D));\n";
    }
    return src + in1 + "}\n";
}

// THE translation of a step into the reference's statements in the reference's order: per result row of a list
// acc = d; acc = acc +- (l * r)[ * c]; d = acc, one piece per row; the element-wise arms, `chunk` statements per piece.
void step_statements(const SlabLayout& lay, const Step& s, const StmtStyle& st, const CodeText& ct, const StmtSink& sink) {
    const uint32_t rb = uint32_t(lay.base_of(s.res));
    std::vector<std::string> ew;   // element-wise statements
    switch (s.kind) {
    case Step::ZERO:
        for (int64_t o = 0; o < lay.plan.layout(s.res).row_len; ++o) ew.push_back(st.el(rb + uint32_t(o)) + " = T(0);");
        break;
    case Step::AXPY:
        for (uint32_t m : s.axpy_map) {
            const std::string d = st.el(rb + (m & 0xffffu));
            ew.push_back(d + " = " + (s.beta ? d : std::string("T(0)")) + " + " + st.el(uint32_t(lay.base_of(s.a)) + (m >> 16)) + ";");
        }
        break;
    case Step::FLIP:
        for (uint32_t o : s.flip_offsets) ew.push_back(st.el(rb + o) + " = -" + st.el(rb + o) + ";");
        break;
    case Step::SUNARY: {
        const std::string d = st.el(rb + uint32_t(s.sunary_off));
        ew.push_back(s.sunary_op == 0 ? d + " = T(1) / " + d + ";" : d + (ct.f32 ? " = __builtin_sqrtf(" : " = __builtin_sqrt(") + d + ");");
        break;
    }
    case Step::DUAL:   // the sign is folded into the operand: d = d + (-x)
        s.dual.for_each([&](uint32_t r, uint32_t a, bool neg) {
            const std::string d = st.el(rb + r), x = st.el(uint32_t(lay.base_of(s.a, s.canon_a)) + a);
            ew.push_back(d + " = " + (s.beta ? d : std::string("T(0)")) + " + " + (neg ? "(-" + x + ")" : x) + ";");
        });
        break;
    case Step::EXPLOG: sink(0, explog_statements(lay, s, st, ct)); break;
    case Step::EXPLOG_ADJ: sink(0, explog_adj_statements(lay, s, st, ct)); break;
    case Step::PRODUCT_CSR: {
        const uint32_t lb = uint32_t(lay.base_of(s.a, s.canon_a)), rrb = uint32_t(lay.base_of(s.b, s.canon_b));
        for (size_t row = 0; row + 1 < s.list.row_start.size(); ++row) {
            const std::string d = st.el(rb + s.list.row_out[row]);
            std::string blk = st.indent + "{ T acc = " + (s.beta ? d : std::string("T(0)")) + ";\n";
            for (uint32_t e = s.list.row_start[row]; e < s.list.row_start[row + 1]; ++e) {
                const std::string prod = "(" + st.el(lb + (s.list.entries[e] & 0xffffu)) + " * " + st.el(rrb + (s.list.entries[e] >> 16)) + ")";
                const double c = s.list.coeff[e];
                blk += st.indent + (c == 1.0 ? "  acc = acc + " + prod : c == -1.0 ? "  acc = acc - " + prod : "  acc = acc + " + prod + " * T(" + ct.lit(c) + ")") + ";\n";
            }
            sink(uint64_t(s.list.row_start[row + 1] - s.list.row_start[row]) + 2, blk + st.indent + "  " + d + " = acc; }\n");
        }
        break;
    }
    default: break;
    }
    for (size_t i = 0; i < ew.size(); i += st.chunk) {
        const size_t cnt = std::min(st.chunk, ew.size() - i);
        std::string blk;
        for (size_t k = i; k < i + cnt; ++k) blk += st.indent + ew[k] + "\n";
        sink(cnt, blk);
    }
}

// ---- the slab in registers, one item per lane
//
// Row I/O.  lane <-> item, but a lane reading ITS row with 16-byte accesses makes every wave instruction touch 64
// different 128-byte lines: the CU's L1 then spends a cycle pair per line for 16 useful bytes and bounds the kernel
// (config 5: 56 % of HBM peak with the vector units 30 % busy).  So a wave (= a workgroup of 64 lanes) moves the
// rows of its 64 items as ONE contiguous span with fully coalesced 16-byte accesses and transposes through LDS:
// rows padded to an odd number of 16-byte units, so that both the span-ordered and the row-per-lane accesses are
// conflict-free.  Used per operand when its rows are contiguous (stride == length) and 16-byte aligned and the wave
// is full; otherwise (shared rows, strided or unaligned wrapped memory, the last partial wave) the lane reads its row
// directly.  GAAST_FLAG_NO_COALESCE: always the direct form (A/B measurements).
constexpr bool kNtStores = (GAAST_JIT_NT & 1) != 0, kNtLoads = (GAAST_JIT_NT & 2) != 0;
std::string load16(const std::string& lvalue, const std::string& ptr) { return kNtLoads ? "__builtin_nontemporal_load(" + ptr + ")" : lvalue; }
std::string store16(const std::string& lvalue, const std::string& ptr, const std::string& value) {
    return kNtStores ? "__builtin_nontemporal_store(" + value + ", " + ptr + ");\n" : lvalue + " = " + value + ";\n";
}
std::string aligned16(const std::string& ptr) { return "(((unsigned long long)" + ptr + ") & 15ull) == 0"; }

struct RowIo {
    const SlabLayout& lay;
    size_t esz;
    int epc;                       // elements per 16-byte chunk
    std::vector<int> lds_off;      // per input: where its span is transposed, -1: not staged
    std::vector<char> by_line;     // per input: 128 bytes of every row at a time through the shared buffer
    bool out_via_lds = false, out_line = false, coalesce = false;
    size_t line_off = 0, lds_total = 0;
    int line_plen;                 // padded line in elements: 9 x 16 bytes, odd -> conflict-free both ways
    int out_len;

    explicit RowIo(const SlabLayout& l);
    static std::string v(uint32_t i) { return "v" + str(i); }
    int padded_len(int len) const {   // row length in LDS, elements
        size_t padb = (size_t(len) * esz + 15) / 16 * 16;
        if ((padb / 16) % 2 == 0) padb += 16;
        return int(padb / esz);
    }
    // the wave's rows as one span of 16-byte chunks: chunk lane + 64 j holds elements el ... el + epc - 1 of the flattened range
    struct Span {
        int len, plen, nch, per_lane;
        bool whole;   // a chunk never straddles two rows
    };
    Span span(int len) const {
        const int nch = 64 * len / epc;   // (64 * len * esz is a multiple of 256)
        return {len, padded_len(len), nch, (nch + 63) / 64, (size_t(len) * esz) % 16 == 0};
    }
    static std::string span_guard(const Span& sp, int j) { return (j + 1) * 64 > sp.nch ? "if (lane + " + str(64 * j) + " < " + str(sp.nch) + ") " : ""; }
    // where element `el` of the span sits in the transposed image
    static std::string span_at(const Span& sp, const std::string& el) { return "(" + el + " / " + str(sp.len) + ") * " + str(sp.plen) + " + " + el + " % " + str(sp.len); }
    // every chunk of a lane: head(j); then body(j, -1, place of the chunk in the image) when chunks are whole, else body(j, e, place of
    // its element e) per element; then tail(j)
    using PerChunk = std::function<std::string(int)>;
    using PerPlace = std::function<std::string(int, int, const std::string&)>;
    std::string span_chunks(const Span& sp, const PerChunk& head, const PerPlace& body, const PerChunk& tail) const {
        std::string src;
        for (int j = 0; j < sp.per_lane; ++j) {
            src += "    " + span_guard(sp, j) + "{ const int el = (lane + " + str(64 * j) + ") * " + str(epc) + ";\n" + head(j);
            if (sp.whole) src += body(j, -1, span_at(sp, "el"));
            for (int e = 0; e < epc && !sp.whole; ++e) src += body(j, e, span_at(sp, "(el + " + str(e) + ")"));
            src += tail(j) + "    }\n";
        }
        return src;
    }
    // the 128-byte blocks of a row of `len` elements
    struct Block {
        int cpl, elems, e0;   // 16-byte chunks, elements, first element
    };
    std::vector<Block> blocks(int len) const {
        std::vector<Block> out;
        for (size_t b = 0; b * 128 < size_t(len) * esz; ++b) {
            const int bytes = int(std::min<size_t>(128, size_t(len) * esz - 128 * b));
            out.push_back({bytes / 16, int(bytes / esz), int(128 * b / esz)});
        }
        return out;
    }
    std::string line_open(const std::string& ptr, const std::string& stride) const {
        return "  if (full && ((" + stride + " * " + str(esz) + ") & 15) == 0 && " + aligned16(ptr) + ") {\n    T* buf = (T*)(lds + " + str(line_off) + ");\n";
    }
    // lane's chunk of row 8 j + (lane >> 3): in the shared buffer, in memory
    std::string line_in_buf(int j) const { return "(buf + (" + str(8 * j) + " + (lane >> 3)) * " + str(line_plen) + " + (lane & 7) * " + str(epc) + ")"; }
    static std::string line_in_mem(int j, const std::string& stride) { return "(base + (long long)(" + str(8 * j) + " + (lane >> 3)) * " + stride + ")"; }
    std::string line_base(const std::string& ptr, const std::string& stride, int e0) const { return ptr + " + item0 * " + stride + " + " + str(e0) + " + (lane & 7) * " + str(epc) + ";\n"; }

    std::string input(size_t i) const;
    std::string output() const;
};

RowIo::RowIo(const SlabLayout& l) : lay(l), esz(l.elem), epc(int(16 / l.elem)), lds_off(l.inputs.size(), -1), by_line(l.inputs.size(), 0),
                                    line_plen(int(144 / l.elem)), out_len(int(l.plan.out_layout.row_len)) {
    const Plan& plan = lay.plan;
    // which operands go through LDS: largest rows first, within a budget that keeps 16 waves per CU resident
    // (160 KiB / 16 = 10 KiB per wave); the result rows reuse the operands' space.  Operands left out (and rows
    // too long for the budget) are read by their lanes directly.
    const size_t lds_budget = (plan.flags & GAAST_FLAG_DEBUG_LDS_12K) ? 12 * 1024 + 256 : 10 * 1024;
    size_t lds_in = 0;
    std::vector<size_t> order(lay.inputs.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return lay.input_len(x) > lay.input_len(y); });
    for (size_t i : order) {
        const size_t need = size_t(64) * size_t(padded_len(lay.input_len(i))) * esz;
        if (lds_in + need > lds_budget) continue;
        lds_off[i] = int(lds_in);
        lds_in += need;
    }
    const size_t lds_out_need = size_t(64) * size_t(padded_len(out_len)) * esz;
    out_via_lds = lds_out_need <= lds_budget;
    // Rows too long for the budget go through ONE shared 64 x 144-byte buffer, 128 bytes (a cache line) of every
    // row at a time: 8 lanes move one row's line, a wave instruction 8 whole lines (so the rows need not even be
    // contiguous, only 16-byte aligned with a 16-byte multiple stride).  Lines of a row are consumed one after the
    // other: a few more barriers (single-wave workgroups: cheap), the same coalescing.
    // (programs with big slabs are register-bound: the transposition's temporaries would spill -- measured on full R^6
    // f32 products, 193 elements: 1.93 -> 1.30 TB/s -- so they keep the row-per-lane form)
    auto line_ok = [&](int len) { return lay.slab <= 128 && size_t(len) * esz >= 128 && (size_t(len) * esz) % 16 == 0; };
    bool any_line = false;
    for (size_t i = 0; i < lay.inputs.size(); ++i)
        if (lds_off[i] < 0 && line_ok(lay.input_len(i))) by_line[i] = 1, any_line = true;
    const bool out_by_line = !out_via_lds && line_ok(out_len);
    any_line = any_line || out_by_line;
    const size_t line_bytes = any_line ? size_t(64) * 144 : 0;
    if (any_line && lds_in + line_bytes > 12 * 1024 + 1024) {   // keep >= 12 waves per CU resident: drop the line path
        std::fill(by_line.begin(), by_line.end(), 0);
        any_line = false;
    }
    line_off = lds_in;                      // the shared line buffer sits after the span regions
    out_line = any_line && out_by_line;
    lds_total = std::max(lds_in + (any_line ? line_bytes : 0), out_via_lds ? lds_out_need : size_t(0));
    coalesce = !(plan.flags & GAAST_FLAG_NO_COALESCE) && lds_total > 0;
}

// the statements that fill input i's slab elements from its rows
std::string RowIo::input(size_t i) const {
    const Step::FusedInput& fi = lay.inputs[i];
    const int len = lay.input_len(i);
    const std::string I = str(i), in = "in" + I, stride = "s" + I;
    auto from_r = [&](const std::string& indent, int first, int count) {   // slab elements first ... <- r[0 ...]
        std::string s;
        for (int c = 0; c < count; ++c) s += indent + v(uint32_t(fi.base + first + c)) + (fi.canon ? " = T(0) + r[" : " = r[") + str(c) + "];\n";
        return s;
    };
    const std::string own_row = "const T* r = " + in + " + item * " + stride + ";\n" + from_r("    ", 0, len) + "  }\n";   // the lane reads its own row
    if (!coalesce) return "  { " + own_row;
    std::string src;
    if (by_line[i]) {   // one cache line of every row at a time through the shared buffer
        src += line_open(in, stride);
        for (const Block& b : blocks(len)) {
            src += "    { const T* base = " + line_base(in, stride, b.e0);
            for (int j = 0; j < 8; ++j) src += "      VT c" + str(j) + ";\n";
            src += "      if ((lane & 7) < " + str(b.cpl) + ") {\n";
            for (int j = 0; j < 8; ++j) {
                const std::string ptr = "(const VT*)" + line_in_mem(j, stride);
                src += "        c" + str(j) + " = " + load16("*" + ptr, ptr) + ";\n";
            }
            for (int j = 0; j < 8; ++j) src += "        *(VT*)" + line_in_buf(j) + " = c" + str(j) + ";\n";
            src += "      }\n      __syncthreads();\n      const T* r = buf + lane * " + str(line_plen) + ";\n";
            src += from_r("      ", b.e0, b.elems);
            src += "      __syncthreads();\n    }\n";
        }
        return src + "  } else if (live) {\n    " + own_row;
    }
    if (lds_off[i] < 0) return "  if (live) { " + own_row;   // not staged
    const Span sp = span(len);
    src += "  if (full && " + stride + " == " + str(len) + " && " + aligned16(in) + ") {\n";
    src += "    const VT* src" + I + " = (const VT*)(" + in + " + item0 * " + str(len) + ");\n";
    src += "    T* img = (T*)(lds + " + str(lds_off[i]) + ");\n";
    for (int j = 0; j < sp.per_lane; ++j) src += "    VT c" + str(j) + ";\n";
    for (int j = 0; j < sp.per_lane; ++j) {
        const std::string at = "src" + I + "[lane + " + str(64 * j) + "]";
        src += "    " + span_guard(sp, j) + "c" + str(j) + " = " + load16(at, "&" + at) + ";\n";
    }
    auto none = [](int) { return std::string(); };
    src += span_chunks(sp, none, [&](int j, int e, const std::string& at) {
        return e < 0 ? "      *(VT*)(img + " + at + ") = c" + str(j) + ";\n" : "      img[" + at + "] = c" + str(j) + "[" + str(e) + "];\n";
    }, none);
    src += "    __syncthreads();\n    const T* r = img + lane * " + str(sp.plen) + ";\n" + from_r("    ", 0, len);
    return src + "  } else if (live) {\n    " + own_row;
}

// the statements that write the result row from its slab elements
std::string RowIo::output() const {
    auto to = [&](const std::string& indent, const char* row, int first, int count) {   // row[0 ...] <- slab elements first ...
        std::string s;
        for (int c = 0; c < count; ++c) s += indent + row + "[" + str(c) + "] = " + v(uint32_t(lay.out_base + first + c)) + ";\n";
        return s;
    };
    if (!coalesce) return "  T* o = out + item * so;\n" + to("  ", "o", 0, out_len);
    std::string src;
    if (out_line) {
        src += line_open("out", "so");
        for (const Block& b : blocks(out_len)) {
            src += "    { __syncthreads();\n      T* r = buf + lane * " + str(line_plen) + ";\n" + to("      ", "r", b.e0, b.elems);
            src += "      __syncthreads();\n      T* base = " + line_base("out", "so", b.e0);
            src += "      if ((lane & 7) < " + str(b.cpl) + ") {\n";
            for (int j = 0; j < 8; ++j) {
                const std::string ptr = "(VT*)" + line_in_mem(j, "so");
                src += "        " + store16("*" + ptr, ptr, "*(const VT*)" + line_in_buf(j));
            }
            src += "      }\n    }\n";
        }
        src += "  } else\n";
    }
    const Span sp = span(out_len);
    src += std::string("  if (") + (out_via_lds ? "full" : "false") + " && so == " + str(out_len) + " && " + aligned16("out") + ") {\n";
    src += "    __syncthreads();\n    T* img = (T*)lds;\n    { T* r = img + lane * " + str(sp.plen) + ";\n" + to("      ", "r", 0, out_len);
    src += "    }\n    __syncthreads();\n    VT* dst = (VT*)(out + item0 * " + str(out_len) + ");\n";
    src += span_chunks(
        sp, [](int) { return std::string("      VT c;\n"); },
        [&](int, int e, const std::string& at) { return e < 0 ? "      c = *(const VT*)(img + " + at + ");\n" : "      c[" + str(e) + "] = img[" + at + "];\n"; },
        [&](int j) { const std::string at = "dst[lane + " + str(64 * j) + "]"; return "      " + store16(at, "&" + at, "c"); });
    return src + "  } else if (live) {\n    T* o = out + item * so;\n" + to("    ", "o", 0, out_len) + "  }\n";
}

void emit_register_form(const SlabLayout& lay, Step& f) {
    const Plan& plan = lay.plan;
    const CodeText ct{plan.dtype == GAAST_F32};
    const RowIo io(lay);
    const int threads = io.coalesce ? 64 : 256;
    std::string src = std::string("typedef ") + ct.ty() + " T;\n";
    src += std::string("typedef ") + ct.ty() + " VT __attribute__((ext_vector_type(" + str(io.epc) + ")));\n";
    src += "extern \"C\" __global__ __launch_bounds__(" + str(threads) + ") void gaast_jit(" + ct.signature(lay.inputs.size()) +
           (plan.has_explog ? ", unsigned long long* dom" : "") + ") {\n";
    if (io.coalesce) {
        src += "  __shared__ __attribute__((aligned(16))) unsigned char lds[" + str(io.lds_total) + "];\n";
        src += "  const int lane = threadIdx.x;\n  const long long item0 = blockIdx.x * 64LL;\n";
        src += "  const long long item = item0 + lane;\n  const bool live = item < batch;\n  const bool full = item0 + 64 <= batch;\n";
    } else {
        src += "  const long long item = blockIdx.x * 256LL + threadIdx.x;\n  if (item >= batch) return;\n";
    }
    for (int i = 0; i < lay.slab; ++i) src += "  T " + RowIo::v(uint32_t(i)) + " = 0;\n";   // every slab element is a local scalar (a register)
    for (size_t i = 0; i < lay.inputs.size(); ++i) src += io.input(i);
    const StmtStyle style{RowIo::v, "  ", 1};
    for (const Step& s : plan.steps) step_statements(lay, s, style, ct, [&](uint64_t, const std::string& text) { src += text; });
    src += io.output() + "}\n";
    f.fused.jit_threads = threads;
    f.fused.jit_source = std::move(src);
    f.fused.jit_reg_trial = lay.slab > lay.jit_slab_small;
}

// ---- MEDIUM programs (round 4): the slab is beyond the registers of the specialised kernel above (160 / 200 elements) but the
// program is short -- the versor inverse a.rev() * a.norm_sq().sinv() at n = 8 (slab 259, 256 comp-muls), the projection KAT at
// n = 12 (slab 171) -- and used to run on the LDS interpreter (wave-uniform micro-op decode: 0.16 / 0.10 of the HBM roof).  The
// same plan as straight-line code over slabs that STAY IN LDS: a workgroup of eight waves owns the slabs of 64 items (item i at
// i * stride elements, stride odd: the lanes of a wave touch 64 different banks at any slab offset), lane <-> item, and the
// independent rows of every arm are dealt to the waves, least-loaded first -- exactly the interpreter's schedule, with the
// decode done by hiprtc: offsets are immediates of the LDS instructions, signs are operators.  Same statements, same order.
struct LdsForm {
    const SlabLayout& lay;
    int stride, epc;
    // chunk k of a thread: 16-byte piece tid + 512 k of a flattened range of 64 rows
    static std::string piece(int k) { return "tid + " + str(512 * k); }
    std::string staging() const;
    std::string step(const Step& s, const CodeText& ct) const;
    std::string output() const;
};

// inputs: element e = item * len + c of the flattened range.  Contiguous, 16-byte aligned rows of a full group of 64 items are
// moved as 16-byte pieces through registers, ALL of them in flight at once, and -- the workgroups are persistent -- the NEXT
// group's pieces are requested before this group is evaluated (a group is 64 KiB at slab 259: the HBM latency hides under
// the arithmetic); anything else -- shared rows, strided wrapped memory, the last partial group -- takes a plain loop
std::string LdsForm::staging() const {
    const size_t n_in = lay.inputs.size();
    std::string src, fast_cond = "true";
    int total_chunks_per_thread = 0;
    for (size_t i = 0; i < n_in; ++i) {
        const int len = lay.input_len(i);
        fast_cond += " && s" + str(i) + " == " + str(len) + " && " + aligned16("in" + str(i));
        if ((64 * len) % epc) fast_cond += " && false";
        total_chunks_per_thread += (64 * len / epc + 511) / 512;
    }
    if (total_chunks_per_thread > 24) fast_cond = "false";
    src += "  const bool fast = " + fast_cond + ";\n";
    src += "  const long long groups = (batch + 63) / 64;\n";
    auto nch = [&](size_t i) { return 64 * lay.input_len(i) / epc; };
    auto cpt = [&](size_t i) { return (nch(i) + 511) / 512; };
    auto to_slab = [&](const Step::FusedInput& fi) { return "slab[i2 * " + str(stride) + " + " + str(fi.base) + " + c] = " + (fi.canon ? "T(0) + v" : "v") + "; }\n"; };
    for (size_t i = 0; i < n_in; ++i) src += "  VT r" + str(i) + "[" + str(std::max(1, cpt(i))) + "];\n";
    src += "  auto issue = [&](long long item0) {\n";
    for (size_t i = 0; i < n_in; ++i) {
        src += "    { const VT* src = (const VT*)(in" + str(i) + " + item0 * " + str(lay.input_len(i)) + ");\n";
        for (int k = 0; k < cpt(i); ++k)
            src += "      if (" + piece(k) + " < " + str(nch(i)) + ") r" + str(i) + "[" + str(k) + "] = __builtin_nontemporal_load(src + " + piece(k) + ");\n";
        src += "    }\n";
    }
    src += "  };\n";
    src += "  auto commit = [&]() {\n";
    for (size_t i = 0; i < n_in; ++i) {
        const std::string L = str(lay.input_len(i));
        for (int k = 0; k < cpt(i); ++k) {
            src += "    if (" + piece(k) + " < " + str(nch(i)) + ") {\n";
            for (int j = 0; j < epc; ++j)
                src += "      { const int e = (" + piece(k) + ") * " + str(epc) + " + " + str(j) + ", i2 = e / " + L + ", c = e - i2 * " + L + "; const T v = r" + str(i) + "[" +
                       str(k) + "][" + str(j) + "]; " + to_slab(lay.inputs[i]);
            src += "    }\n";
        }
    }
    src += "  };\n";
    src += "  auto stage = [&](long long item0, int nitems) {\n";
    for (size_t i = 0; i < n_in; ++i) {
        const std::string I = str(i), L = str(lay.input_len(i));
        src += "#pragma unroll 4\n    for (int e = tid; e < " + str(64 * lay.input_len(i)) + "; e += 512) { const int i2 = e / " + L + ", c = e - i2 * " + L +
               "; T v = i2 < nitems ? in" + I + "[(item0 + i2) * s" + I + " + c] : T(0); " + to_slab(lay.inputs[i]);
    }
    return src + "  };\n";
}

// one arm: its independent pieces dealt to the waves, least-loaded first, then a barrier
std::string LdsForm::step(const Step& s, const CodeText& ct) const {
    std::string per_wave[uop::GROUPS];
    WaveLoads waves;
    const StmtStyle style{[](uint32_t i) { return "my[" + str(i) + "]"; }, "      ", 16};
    step_statements(lay, s, style, ct, [&](uint64_t cost, const std::string& text) { per_wave[waves.take(cost)] += text; });
    std::string src = "  switch (wave) {\n";
    for (int g = 0; g < uop::GROUPS; ++g)
        if (!per_wave[g].empty()) src += "    case " + str(g) + ": {\n" + per_wave[g] + "    } break;\n";
    return src + "    default: break;\n  }\n  __syncthreads();\n";
}

std::string LdsForm::output() const {
    const int out_len = int(lay.plan.out_layout.row_len);
    const int nch = 64 * out_len / epc, cpt = (nch + 511) / 512;
    const std::string OL = str(out_len), from_slab = "slab[i2 * " + str(stride) + " + " + str(lay.out_base) + " + c]";
    std::string src = "  if (nitems == 64 && so == " + OL + " && " + aligned16("out") + " && " + ((64 * out_len) % epc == 0 && cpt <= 24 ? "true" : "false") + ") {\n";
    src += "    VT* dst = (VT*)(out + item0 * " + OL + ");\n";
    for (int k = 0; k < cpt; ++k) {
        src += "    if (" + piece(k) + " < " + str(nch) + ") { VT v;\n";
        for (int j = 0; j < epc; ++j)
            src += "      { const int e = (" + piece(k) + ") * " + str(epc) + " + " + str(j) + ", i2 = e / " + OL + ", c = e - i2 * " + OL + "; v[" + str(j) + "] = " + from_slab + "; }\n";
        src += "      __builtin_nontemporal_store(v, dst + " + piece(k) + "); }\n";
    }
    src += "  } else {\n";
    src += "#pragma unroll 4\n    for (int e = tid; e < " + str(64 * out_len) + "; e += 512) { const int i2 = e / " + OL + ", c = e - i2 * " + OL +
           "; if (i2 < nitems) out[(item0 + i2) * so + c] = " + from_slab + "; }\n";
    return src + "  }\n";
}

void emit_lds_form(const SlabLayout& lay, Step& f) {
    const Plan& plan = lay.plan;
    const CodeText ct{plan.dtype == GAAST_F32};
    const LdsForm form{lay, lay.slab | 1, int(16 / lay.elem)};
    std::string src = std::string("typedef ") + ct.ty() + " T;\n";
    src += "extern \"C\" __global__ __launch_bounds__(512) void gaast_jit(" + ct.signature(lay.inputs.size()) + ") {\n";
    src += "  __shared__ T slab[" + str(64 * form.stride) + "];\n";
    src += "  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;\n";
    src += "  T* const my = slab + lane * " + str(form.stride) + ";\n";
    src += "  typedef T VT __attribute__((ext_vector_type(" + str(form.epc) + ")));\n";
    src += form.staging();
    src += R"(  long long g = blockIdx.x;
  if (g >= groups) return;
  { const long long item0 = g * 64; const int nitems = int(batch - item0 < 64 ? batch - item0 : 64);
    if (fast && nitems == 64) { issue(item0); commit(); } else stage(item0, nitems); }
  for (;;) {
  const long long item0 = g * 64;
  const int nitems = int(batch - item0 < 64 ? batch - item0 : 64);
  const long long gn = g + gridDim.x;
  const bool more = gn < groups;
  const int nnext = more ? int(batch - gn * 64 < 64 ? batch - gn * 64 : 64) : 0;
  const bool pre_next = fast && more && nnext == 64;
  __syncthreads();
  if (pre_next) issue(gn * 64);
)";
    for (const Step& s : plan.steps) src += form.step(s, ct);
    src += form.output();
    src += "  if (!more) break;\n  g = gn;\n  __syncthreads();\n";   // the slabs are rewritten for the next group
    src += "  if (pre_next) commit(); else stage(gn * 64, nnext);\n";
    src += "  }\n";
    src += "}\n";
    f.fused.jit_threads = 512;
    f.fused.jit_items = 64;
    f.fused.jit_persistent = int(std::max<size_t>(1, kLdsBytes / (size_t(64) * size_t(form.stride) * lay.elem)));   // workgroups resident per CU (LDS)
    f.fused.jit_source = std::move(src);
}

}  // namespace

int fused_slab(const Plan& plan, bool small_reg_slab) {
    const SlabLayout lay(plan, small_reg_slab);
    return lay.ok ? lay.slab : 0;
}

bool try_fuse(Plan& plan, bool small_reg_slab) {
    const SlabLayout lay(plan, small_reg_slab);
    if (!lay.ok) return false;
    Step f;
    f.kind = Step::FUSED;
    f.res = BufRef{BufKind::OUT, 0};
    f.fused.inputs = lay.inputs;
    uint64_t entries = 0;
    if (!encode_uops(lay, f.fused, entries)) return false;
    if (!lay.interp_ok && entries > 8192) return false;
    f.fused.jit_only = lay.interp_ok ? 0 : 1;
    // exp / log steps (no interpreter micro-ops, plan.has_explog) exist in the register form only: it or nothing
    if (lay.jit_allowed && entries <= 8192)
        emit_register_form(lay, f);
    else if (!(plan.flags & GAAST_FLAG_NO_JIT) && lay.interp_ok && !plan.has_explog && !plan.has_explog_adj && entries <= 2048 && size_t(lay.slab | 1) * lay.elem * 64 + 64 <= kLdsBytes)
        emit_lds_form(lay, f);
    f.fused.slab = lay.slab;
    f.fused.zero_slot = lay.zero_slot;
    f.fused.out_base = lay.out_base;
    f.n_entries = entries;
    f.name = "ast_fused[" + std::to_string(plan.steps.size()) + " arms, " + std::to_string(entries) +
             " comp-muls, slab " + std::to_string(lay.slab) + "]";
    plan.steps.clear();
    plan.steps.push_back(std::move(f));
    plan.node_buffers.clear();  // the cache buffers live in LDS now
    return true;
}

}  // namespace gaast
