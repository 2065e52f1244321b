// The whole-plan rewrite passes that run after the lowering walk (plan.cpp) on a plan that was not fused into one small-program
// launch (plan_fused.cpp).  See plan_internal.hpp: run_plan_passes.
#include "plan_internal.hpp"

#include <algorithm>

namespace gaast {
namespace {

// Who uses a buffer.  The only step that writes `buf`, when it comes before step `reader` and no step but `reader` reads the buffer;
// else -1.  (What else a pass asks of the writer -- its kind, beta, form -- it says where it calls.)
int sole_writer(const Plan& plan, BufRef buf, size_t reader) {
    int writer = -1;
    for (size_t i = 0; i < plan.steps.size(); ++i) {
        if (i == reader) continue;
        const Step& t = plan.steps[i];
        if (reads(t, buf) || (t.res == buf && (writer >= 0 || i > reader))) return -1;
        if (t.res == buf) writer = int(i);
    }
    return writer;
}
// ... no step outside first .. last reads or writes `buf`
bool untouched_outside(const Plan& plan, BufRef buf, size_t first, size_t last) {
    for (size_t k = 0; k < plan.steps.size(); ++k)
        if ((k < first || k > last) && (plan.steps[k].res == buf || reads(plan.steps[k], buf))) return false;
    return true;
}
// ... the operands of step `writer` still hold at step `reader`: inputs always do; a cache buffer does unless a step between the two
// writes it (cache buffers are written by the steps that fill them, all before their first reader)
bool operands_hold(const Plan& plan, size_t writer, size_t reader) {
    const Step& w = plan.steps[writer];
    for (size_t i = writer + 1; i < reader; ++i)
        if (plan.steps[i].res == w.a || plan.steps[i].res == w.b) return false;
    return true;
}
bool any_fused(const Plan& plan) {
    return std::any_of(plan.steps.begin(), plan.steps.end(), [](const Step& t) { return t.kind == Step::FUSED; });
}

// The ELL form of a comp-mul list.  The width of its rows when they have one length and every coefficient is +-1; else 0
uint32_t ell_width(const std::vector<uint32_t>& row_start, const std::vector<double>& coeff) {
    const size_t rows = row_start.empty() ? 0 : row_start.size() - 1;
    const uint32_t width = rows ? row_start[1] - row_start[0] : 0;
    for (size_t r = 0; r < rows; ++r)
        if (row_start[r + 1] - row_start[r] != width) return 0;
    for (double c : coeff)
        if (c != 1.0 && c != -1.0) return 0;
    return width;
}
// ... and its words transposed to [term][row], the sign in bit 31; terms width .. padded - 1 of every row are pad_word
std::vector<uint32_t> ell_words(const std::vector<uint32_t>& row_start, const std::vector<uint32_t>& entries, const std::vector<double>& coeff, uint32_t width,
                                uint32_t padded, uint32_t pad_word) {
    const size_t rows = row_start.size() - 1;
    std::vector<uint32_t> ell(size_t(padded) * rows, pad_word);
    for (size_t r = 0; r < rows; ++r)
        for (uint32_t t = 0; t < width; ++t) {
            const size_t e = size_t(row_start[r]) + t;
            ell[size_t(t) * rows + r] = entries[e] | (coeff[e] < 0.0 ? 0x80000000u : 0u);
        }
    return ell;
}

// The only writer of Plan::node_dead (sized by build_plan): no step touches cache buffer `buf` any more, it is never allocated
void mark_dead(Plan& plan, BufRef buf) { plan.node_dead[size_t(buf.idx)] = 1; }

// Steps first .. last - 1 leave the plan (their work rides in another step now)
void drop_steps(Plan& plan, size_t first, size_t last) { plan.steps.erase(plan.steps.begin() + ptrdiff_t(first), plan.steps.begin() + ptrdiff_t(last)); }

}  // namespace

// Rows of one length with +-1 coefficients (dense products of non-degenerate algebras) that were not fused
// into a small-program launch: the same lists transposed to [term][row] with the sign in bit 31 --
// consecutive threads (rows) then read consecutive words and no coefficient array is streamed
// (k_product_ell).  Same order, same roundings: (l * r) * (-1.0) is -(l * r) exactly.
void uniform_csr_to_ell(Plan& plan) {
    if (plan.flags & GAAST_FLAG_NO_FUSION) return;
    for (Step& s : plan.steps) {
        if (s.kind != Step::PRODUCT_CSR || s.list.row_out.empty()) continue;
        const uint32_t width = ell_width(s.list.row_start, s.list.coeff);
        bool uniform = width >= 4;   // (round 3: from 4 terms per row on -- R X has n per row; 16 before: such lists ran on k_product_csr, an entry and a coefficient load per term)
        for (size_t e = 0; uniform && e < s.list.entries.size(); ++e) uniform = !(s.list.entries[e] & 0x80000000u);   // right offset < 2^15
        if (!uniform) continue;
        // offsets in BYTES when they fit 15 bits (rows of <= 32 KiB: n <= 12 in f64, n <= 13 in f32): the kernel
        // then adds them to an LDS base without scaling
        const uint32_t elem = plan.dtype == GAAST_F32 ? 4u : 8u;
        bool bytes = true;
        for (size_t e = 0; bytes && e < s.list.entries.size(); ++e)
            bytes = (s.list.entries[e] & 0xffffu) * elem < 32768u && (s.list.entries[e] >> 16) * elem < 32768u;
        if (bytes)
            for (uint32_t& e : s.list.entries) e = ((e & 0xffffu) * elem) | ((e >> 16) * elem << 16);
        s.list.entries = ell_words(s.list.row_start, s.list.entries, s.list.coeff, width, width, 0u);
        s.list.ell_bytes = bytes ? 1 : 0;
        s.list.coeff.clear();
        s.list.ell_width = int(width);
        s.name = "product_ell" + s.name.substr(s.name.find('['));
    }
}

// A sparse product whose result is read ONLY as the left operand of a dense product (R X in R X ~R, eval.rs:61-86 with its
// cached operand) is evaluated inside the dense kernel, in LDS, while that kernel stages its operands: one launch instead of
// two, and the intermediate row never goes through HBM (BASELINE configs[4] at the dimensions where the whole program no
// longer fits a fused small-program kernel).  The list keeps the reference's order and roundings, so the dense kernel sees
// the very bits the separate launch would have written.  Off with GAAST_FLAG_DEBUG_NO_CHAIN (A/B, tests).
static void chain_sparse_into_dense(Plan& plan) {
    if (plan.flags & (GAAST_FLAG_NO_FUSION | GAAST_FLAG_DEBUG_NO_CHAIN)) return;
    if (any_fused(plan)) return;
    const size_t elem = plan.dtype == GAAST_F32 ? 4 : 8;
    for (size_t j = 0; j < plan.steps.size(); ++j) {
        Step& dn = plan.steps[j];
        const DenseFamily fam = dn.dense.family;   // (k_gp_mfma6 has no chained staging: programs that small are fused whole)
        if (dn.kind != Step::PRODUCT_DENSE || fam == DenseFamily::SPINOR || fam == DenseFamily::MFMA6 || dn.dense.chained || dn.a.kind != BufKind::NODE) continue;
        const BufRef buf = dn.a;
        // exactly one writer, a list product that starts the buffer (beta = 0) and whose operands still hold at the dense launch;
        // no other reader
        const int writer = dn.b == buf ? -1 : sole_writer(plan, buf, j);
        if (writer < 0) continue;
        Step& w = plan.steps[size_t(writer)];
        if (w.kind != Step::PRODUCT_CSR || w.beta != 0 || !operands_hold(plan, size_t(writer), j)) continue;
        const int64_t ll = plan.layout(w.a).row_len, rl = plan.layout(w.b).row_len;
        const int n2 = dn.dense.n;
        // items a workgroup of the dense kernel stages at once and its operand images (dense_images::geometry, which the launcher
        // fills its launch from too); 256 bytes stand for the kernel's padding and zero words
        const dense_images::Geometry g = dense_images::geometry(fam, n2, int(elem));
        const int ipb = g.items;
        const size_t scratch = size_t(ipb) * size_t(ll + rl + 1) * elem;
        const size_t images = size_t(ipb) * (size_t(g.images) << n2) * elem + 256;
        if (scratch > 48 * 1024 || images + scratch > kLdsBytes - 1024 || w.list.row_out.size() > 32768) continue;
        // rows of the list -> components of the dense step's left image
        std::vector<int32_t> map_of(size_t(plan.layout(buf).row_len), -1);
        for (size_t c = 0; c < dn.dense.left_map.size(); ++c) map_of[dn.dense.left_map[c] & 0xffffu] = int32_t(c);
        dn.pre.row_map.clear();
        dn.pre.row_scale.clear();
        bool covered = true;
        std::vector<uint32_t> row_start(1, 0u), entries;
        std::vector<double> coeff;
        std::vector<char> produced(dn.dense.left_map.size(), 0);
        for (size_t row = 0; row < w.list.row_out.size(); ++row) {
            const int32_t c = map_of[w.list.row_out[row]];
            if (c < 0) continue;   // a component the dense product does not read (its grade is not wanted there)
            produced[size_t(c)] = 1;
            dn.pre.row_map.push_back(dn.dense.left_map[size_t(c)] & 0xffff0000u);
            if (dn.dense.scaled) dn.pre.row_scale.push_back(dn.dense.left_scale[size_t(c)]);
            for (uint32_t e = w.list.row_start[row]; e < w.list.row_start[row + 1]; ++e) {
                entries.push_back(w.list.entries[e]);
                coeff.push_back(w.list.coeff[e]);
            }
            row_start.push_back(uint32_t(entries.size()));
        }
        for (char c : produced) covered = covered && c;
        // rows of one length with +-1 coefficients (R X: n entries per row): [term][row] words, sign in bit 31
        const uint32_t width = ell_width(row_start, coeff);
        bool uniform = width > 0 && ll + rl + 1 < 0x8000;
        for (size_t e = 0; uniform && e < entries.size(); ++e) uniform = (entries[e] & 0xffffu) < 0x8000u && (entries[e] >> 16) < 0x8000u;
        if (uniform) {
            // padded to a multiple of 4 terms with entries over the zero pair the kernel keeps behind the two rows
            // (left offset ll + rl from the left row, right offset rl from the right row): acc + (+0.0) changes no acc
            const uint32_t wpad = (width + 3u) & ~3u;
            entries = ell_words(row_start, entries, coeff, width, wpad, uint32_t(ll + rl) | (uint32_t(rl) << 16));
            coeff.clear();
            dn.pre.width = int(wpad);
        }
        dn.dense.chained = 1;
        dn.pre.a = w.a;
        dn.pre.b = w.b;
        dn.pre.canon_a = w.canon_a;
        dn.pre.canon_b = w.canon_b;
        dn.pre.row_start = std::move(row_start);
        dn.pre.entries = std::move(entries);
        dn.pre.coeff = std::move(coeff);
        dn.pre.left_len = int(ll);
        dn.pre.right_len = int(rl);
        // components no row produces stay zero: the kernel zero-fills the image first unless every loaded component is covered
        dn.dense.left_full = dn.dense.left_full && covered;
        dn.dense.left_contig = 0;   // general staging
        dn.name += " <- " + w.name + " in LDS";
        dn.n_entries += w.n_entries;
        dn.a = BufRef{BufKind::NODE, -1};
        mark_dead(plan, buf);
        drop_steps(plan, size_t(writer), size_t(writer) + 1);   // (the writer came before: the dense step is now step j - 1)
        --j;
    }
}

// A list product whose result is read ONLY by another list product (as either operand): both run in ONE k_product_ell_chain
// launch with the mid row in LDS -- the rotor sandwich applied to a vector, (R X ~R).g(1), where it no longer fits a fused
// small-program kernel (n >= 9) and its second product (n rows of 2^(n-1) terms) is far too sparse for the dense kernels.  Same
// order, same roundings: bit for bit the two-launch plan.  Off with GAAST_FLAG_DEBUG_NO_CHAIN.
void chain_list_into_list(Plan& plan) {
    if (plan.flags & (GAAST_FLAG_NO_FUSION | GAAST_FLAG_DEBUG_NO_CHAIN)) return;
    if (any_fused(plan)) return;
    const size_t elem = plan.dtype == GAAST_F32 ? 4 : 8;
    auto ell_list = [](const Step& t) { return t.kind == Step::PRODUCT_CSR && t.list.ell_width > 0 && t.list.ell_bytes && !t.chain.side; };
    for (size_t j = 0; j < plan.steps.size(); ++j) {
        Step& c = plan.steps[j];
        if (!ell_list(c)) continue;
        for (int side = 1; side <= 2; ++side) {
            const BufRef buf = side == 1 ? c.a : c.b, other = side == 1 ? c.b : c.a;
            if (buf.kind != BufKind::NODE || buf.idx < 0 || buf == other) continue;
            // exactly one writer, a list of the same form that starts the buffer (beta = 0), does not read it or this list's result,
            // and whose operands still hold at this list; no other reader
            const int writer = sole_writer(plan, buf, j);
            if (writer < 0) continue;
            Step& w = plan.steps[size_t(writer)];
            if (!ell_list(w) || w.beta != 0 || c.res == w.a || c.res == w.b || !operands_hold(plan, size_t(writer), j)) continue;
            const int64_t l1 = plan.layout(w.a).row_len, r1 = plan.layout(w.b).row_len, mid = plan.layout(buf).row_len, r2 = plan.layout(other).row_len;
            const int canon_other = side == 1 ? c.canon_b : c.canon_a;
            int alias = 0;
            if (other == w.a && canon_other == w.canon_a) alias = 1;
            else if (other == w.b && canon_other == w.canon_b) alias = 2;
            const int64_t per_item = l1 + r1 + mid + (alias ? 0 : r2);
            if (per_item * int64_t(elem) >= 32768 * 3) continue;       // byte offsets of the entries stay below 32 KiB per row anyway
            int64_t stride = per_item;
            while (stride % 32 != 1) ++stride;                         // consecutive items: consecutive banks
            // items per workgroup: about 36 KiB of LDS (four workgroups per CU: one's staging overlaps another's lists), at least
            // four items when that still fits the CU
            // this list's words ride in LDS when they take at most 48 KiB (n <= 11 for the sandwich)
            int64_t ent2 = ((int64_t(c.list.ell_width) + 4) * int64_t(c.list.row_out.size()) * 4 + 15) / 16 * 16;   // [row][term], rows 4 words apart; widths are multiples of 4
            if (ent2 > 48 * 1024 || c.list.ell_width % 4) ent2 = 0;
            // items per workgroup: as many as make this list's (row, item) pairs just fill a wave (9 rows: 7 items = 63 lanes) -- a
            // second, nearly empty wave would issue the whole list again --, fewer when the LDS does not hold them
            const int64_t rows2 = int64_t(c.list.row_out.size());
            int64_t ipb = rows2 <= 32 ? 64 / rows2 : 4;
            const int64_t lds_cap = int64_t(kLdsBytes) - 16 * 1024;
            while (ipb > 2 && ent2 + ipb * stride * int64_t(elem) > lds_cap / 2) --ipb;   // two workgroups per CU when that costs at most ...
            if (ipb < 4) {                                                                 // ... down to four items; then one workgroup per CU
                ipb = std::min<int64_t>(rows2 <= 32 ? 64 / rows2 : 4, 4);
                if (ent2 + ipb * stride * int64_t(elem) > lds_cap) ent2 = 0;
                while (ipb > 1 && ipb * stride * int64_t(elem) > lds_cap) --ipb;
            }
            if (ipb < 2 || ent2 + ipb * stride * int64_t(elem) > lds_cap) continue;
            c.chain.ent2_lds = int(ent2);
            // rows of the first list -> their element offsets in the mid row; is every component of the mid row produced?
            std::vector<char> produced(size_t(mid), 0);
            for (uint32_t off : w.list.row_out) produced[off] = 1;
            bool covered = true;
            for (char x : produced) covered = covered && x;
            c.chain.side = side;
            c.chain.alias = alias;
            c.chain.mid_len = int(mid);
            c.chain.canon_mid = side == 1 ? c.canon_a : c.canon_b;
            c.chain.covered = covered ? 1 : 0;
            c.chain.ipb = int(ipb);
            c.chain.item_stride = int(stride);
            c.pre.a = w.a;
            c.pre.b = w.b;
            c.pre.canon_a = w.canon_a;
            c.pre.canon_b = w.canon_b;
            c.pre.left_len = int(l1);
            c.pre.right_len = int(r1);
            c.pre.entries = w.list.entries;
            c.pre.row_map = w.list.row_out;
            c.pre.width = w.list.ell_width;
            c.name += " <- " + w.name + " in LDS";
            c.n_entries += w.n_entries;
            make_chain_jit(plan, c, &w, l1, r1, mid, r2, alias, side, covered);
            (side == 1 ? c.a : c.b) = BufRef{BufKind::NODE, -1};
            mark_dead(plan, buf);
            drop_steps(plan, size_t(writer), size_t(writer) + 1);   // (the first list came before: this one is now step j - 1)
            --j;
            break;
        }
    }
}

// A RUN of element-wise arms on one buffer -- add_grades_from copies / additions of bound inputs, Negation / Reverse / GradeInvolution
// sign flips (eval.rs:45-60, 87-102) -- costs one full read-modify-write of the buffer PER ARM when every arm is a launch
// ((-(a.rev()) + b.ginvol()).rev() * s at n = 12: six passes).  The components never look at each other, so the run becomes ONE
// k_elementwise pass in which each component executes its own statements in program order: bit-identical.  When the run's buffer is
// only the operand of a product of one-term rows with a scalar operand, that product rides along as the pass's epilogue and the
// buffer is never written at all.
static void fuse_elementwise_runs(Plan& plan) {
    if (plan.flags & (GAAST_FLAG_NO_FUSION | GAAST_FLAG_DEBUG_NO_CHAIN)) return;
    for (size_t i = 0; i < plan.steps.size(); ++i) {
        const Step& first = plan.steps[i];
        if (first.kind != Step::AXPY && first.kind != Step::FLIP && first.kind != Step::DUAL) continue;
        const BufRef R = first.res;
        size_t j = i;
        std::vector<BufRef> srcs;
        bool ok = true;
        while (j < plan.steps.size() && ok) {
            const Step& t = plan.steps[j];
            if ((t.kind != Step::AXPY && t.kind != Step::FLIP && t.kind != Step::DUAL) || t.res != R) break;
            if (t.kind != Step::FLIP) {   // AXPY, DUAL: statements that read a bound input
                if (t.a.kind != BufKind::INPUT) break;
                bool known = false;
                for (const BufRef& b : srcs) known = known || b == t.a;
                if (!known) {
                    if (srcs.size() == 6) break;
                    srcs.push_back(t.a);
                }
            }
            ++j;
            if (j - i == 8) break;   // (a pass holds eight statements per component; a longer run continues in a second pass)
        }
        const size_t n_ops = j - i;
        if (n_ops < 2) continue;
        // components the run touches, in row order
        const int64_t rl = plan.layout(R).row_len;
        std::vector<int32_t> comp_of(size_t(rl), -1);
        std::vector<uint32_t> comps;
        for (size_t k = i; k < j; ++k) {
            for (uint32_t w : plan.steps[k].axpy_map) comp_of[w & 0xffffu] = 0;
            for (uint32_t off : plan.steps[k].flip_offsets) comp_of[off] = 0;
            if (plan.steps[k].kind == Step::DUAL) plan.steps[k].dual.for_each([&](uint32_t r, uint32_t, bool) { comp_of[r] = 0; });
        }
        for (int64_t o = 0; o < rl; ++o)
            if (comp_of[size_t(o)] == 0) {
                comp_of[size_t(o)] = int32_t(comps.size());
                comps.push_back(uint32_t(o));
            }
        const size_t nc = comps.size();
        if (nc == 0) continue;
        std::vector<uint32_t> ops(n_ops * nc, 0u);
        for (size_t k = i; k < j; ++k) {
            const Step& t = plan.steps[k];
            if (t.kind == Step::FLIP) {
                for (uint32_t off : t.flip_offsets) ops[(k - i) * nc + size_t(comp_of[off])] = 2u;
            } else {
                uint32_t slot = 0;
                for (size_t q = 0; q < srcs.size(); ++q)
                    if (srcs[q] == t.a) slot = uint32_t(q);
                for (uint32_t w : t.axpy_map) ops[(k - i) * nc + size_t(comp_of[w & 0xffffu])] = (t.beta ? 1u : 3u) | (slot << 2) | ((w >> 16) << 16);
                if (t.kind == Step::DUAL)   // a complement: the same statement with the source negated (bit 5) and read as a product operand (bit 6)
                    t.dual.for_each([&](uint32_t r, uint32_t a, bool neg) {
                        ops[(k - i) * nc + size_t(comp_of[r])] = (t.beta ? 1u : 3u) | (slot << 2) | (neg ? 32u : 0u) | (t.canon_a ? 64u : 0u) | (a << 16);
                    });
            }
        }
        // Every component executes ITS OWN statements in order, so each list is compacted on its own: empty statements go, and two
        // sign flips in a row cancel exactly (-(-x) has the bits of x) -- (-(a.rev()) + b.ginvol()).rev() on grade-6 rows is
        // copy, flip, flip, add, flip: three statements.  Four or fewer statements run on the kernel instantiation with half the
        // registers (k_elementwise<T, 4>).
        {
            std::vector<std::vector<uint32_t>> lists(nc);
            size_t longest = 1;
            for (size_t c = 0; c < nc; ++c) {
                for (size_t k = 0; k < n_ops; ++k) {
                    const uint32_t w = ops[k * nc + c];
                    if ((w & 3u) == 0u) continue;
                    if ((w & 3u) == 2u && !lists[c].empty() && (lists[c].back() & 3u) == 2u) lists[c].pop_back();
                    else lists[c].push_back(w);
                }
                longest = std::max(longest, lists[c].size());
            }
            ops.assign(longest * nc, 0u);
            for (size_t c = 0; c < nc; ++c)
                for (size_t k = 0; k < lists[c].size(); ++k) ops[k * nc + c] = lists[c][k];
        }
        const size_t n_stmt = ops.size() / nc;
        // does every component start with a copy (the run then never reads its buffer)?
        bool load_first = false;
        for (size_t c = 0; c < nc && !load_first; ++c) {
            size_t k = 0;
            while (k < n_stmt && ops[k * nc + c] == 0u) ++k;
            load_first = k == n_stmt || (ops[k * nc + c] & 3u) != 3u;
        }
        Step f;
        f.kind = Step::ELEMENTWISE;
        f.res = R;
        f.ew.src = srcs;
        f.ew.n_ops = int(n_stmt);
        f.ew.load_first = load_first ? 1 : 0;
        f.ew.ops = std::move(ops);
        f.ew.comp_off = comps;
        f.name = "elementwise[" + std::to_string(n_ops) + " arms:";
        for (size_t k = i; k < j; ++k) f.name += " " + plan.steps[k].name.substr(0, plan.steps[k].name.find('[') == std::string::npos ? 8 : plan.steps[k].name.find('['));
        f.name += "]";
        // the scaling product right after the run, reading the run's buffer and a scalar?
        size_t drop_to = j;
        if (R.kind == BufKind::NODE && j < plan.steps.size() && !load_first && int64_t(nc) == rl) {
            const Step& p2 = plan.steps[j];
            const bool r_left = p2.kind == Step::PRODUCT_CSR && p2.a == R, r_right = p2.kind == Step::PRODUCT_CSR && p2.b == R;
            if (p2.kind == Step::PRODUCT_CSR && p2.beta == 0 && r_left != r_right && !p2.chain.side && p2.list.row_out.size() == nc) {
                const BufRef S = r_left ? p2.b : p2.a;
                bool fits = plan.layout(S).row_len == 1 && S != R && p2.res != R;
                for (size_t r = 0; r + 1 < p2.list.row_start.size() && fits; ++r) fits = p2.list.row_start[r + 1] - p2.list.row_start[r] == 1;
                fits = fits && untouched_outside(plan, R, i, j);   // nobody else reads the run's buffer
                std::vector<uint32_t> out_off(nc, 0u);
                std::vector<double> coeff(nc, 0.0);
                std::vector<char> seen(nc, 0);
                for (size_t r = 0; r + 1 < p2.list.row_start.size() && fits; ++r) {
                    const uint32_t e = p2.list.entries[p2.list.row_start[r]];
                    const uint32_t roff = r_left ? (e & 0xffffu) : (e >> 16);
                    fits = roff < uint32_t(rl) && comp_of[roff] >= 0 && !seen[size_t(comp_of[roff])];
                    if (!fits) break;
                    seen[size_t(comp_of[roff])] = 1;
                    out_off[size_t(comp_of[roff])] = p2.list.row_out[r];
                    coeff[size_t(comp_of[roff])] = p2.list.coeff[p2.list.row_start[r]];
                }
                if (fits) {
                    f.ew.scale = 1;
                    f.res = p2.res;
                    f.b = S;
                    f.ew.out_off = std::move(out_off);
                    f.ew.coeff = std::move(coeff);
                    f.ew.scalar_off = 0;
                    f.ew.canon_v = r_left ? p2.canon_a : p2.canon_b;
                    f.ew.canon_s = r_left ? p2.canon_b : p2.canon_a;
                    f.ew.s_is_left = r_left ? 0 : 1;
                    f.beta = 0;
                    f.n_entries = p2.n_entries;
                    f.name += " * scalar -> " + p2.name;
                    mark_dead(plan, R);
                    drop_to = j + 1;
                }
            }
        }
        plan.steps[i] = std::move(f);
        drop_steps(plan, i + 1, drop_to);
    }
}

// x (*) f(<l, r>): a product into ONE scalar component (a single row: norm_sq), an optional ScalarUnaryOp on it, and a product of
// one-term rows that multiplies another row by that scalar -- a.rev() * a.norm_sq().sinv(), the versor inverse of expr.rs:363-371,
// where the rows no longer fit a fused slab -- become ONE k_reduce_scale launch (kernels_exact.hip.hpp): reference order and
// roundings, the scalar never leaves the wave, the row is streamed once from HBM.  Runs on the CSR form, before the ELL pass.
static bool fuse_one_reduce_scale(Plan& plan) {   // the first instance in the plan, if any
    for (size_t i = 0; i + 1 < plan.steps.size(); ++i) {
        Step& p1 = plan.steps[i];
        if (p1.kind != Step::PRODUCT_CSR || p1.list.row_out.size() != 1 || p1.beta != 0 || p1.res.kind != BufKind::NODE || p1.chain.side) continue;
        if (plan.node_buffers[size_t(p1.res.idx)].row_len != 1 || p1.list.entries.size() < 64) continue;
        const BufRef S = p1.res;
        size_t j = i + 1;
        int op = 0;
        if (plan.steps[j].kind == Step::SUNARY && plan.steps[j].res == S && plan.steps[j].sunary_off == 0) {
            op = plan.steps[j].sunary_op == 0 ? 1 : 2;
            ++j;
        }
        if (j >= plan.steps.size()) continue;
        Step& p2 = plan.steps[j];
        if (p2.kind != Step::PRODUCT_CSR || p2.beta != 0 || p2.chain.side) continue;
        const bool s_left = p2.a == S, s_right = p2.b == S;
        if (s_left == s_right) continue;
        const BufRef xop = s_left ? p2.b : p2.a;
        if (xop == S || p2.res == p1.a || p2.res == p1.b || p2.res == xop) continue;
        bool ok = untouched_outside(plan, S, i, j);   // nobody else touches the scalar (steps i .. j: the products and the unary op)
        for (size_t r = 0; r + 1 < p2.list.row_start.size() && ok; ++r) ok = p2.list.row_start[r + 1] - p2.list.row_start[r] == 1;   // one term per row
        for (uint32_t o : p2.list.row_out) ok = ok && o < 65536u;   // out offsets need 16 bits
        if (!ok) continue;
        Step f;
        f.kind = Step::REDUCE_SCALE;
        f.res = p2.res;
        f.a = p1.a;
        f.b = p1.b;
        f.reduce.x = xop;
        f.canon_a = p1.canon_a;
        f.canon_b = p1.canon_b;
        f.reduce.canon_x = s_left ? p2.canon_b : p2.canon_a;
        f.reduce.canon_s = s_left ? p2.canon_a : p2.canon_b;
        f.reduce.op = op;
        f.reduce.s_is_left = s_left ? 1 : 0;
        f.reduce.ent1 = p1.list.entries;
        f.reduce.coeff1 = p1.list.coeff;
        f.reduce.ent2.resize(p2.list.entries.size());
        f.reduce.coeff2 = p2.list.coeff;
        for (size_t r = 0; r + 1 < p2.list.row_start.size(); ++r) {
            const uint32_t e = p2.list.entries[p2.list.row_start[r]];
            const uint32_t xoff = s_left ? (e >> 16) : (e & 0xffffu);
            f.reduce.ent2[r] = xoff | (p2.list.row_out[r] << 16);
        }
        f.beta = 0;
        f.n_entries = p1.n_entries + p2.n_entries;
        // tolerance mode: can a wave keep the row in registers and read it once (k_reduce_scale_wave)?  The reduction must be one term
        // per component, (i, i), coefficient +-1, in any order; the scaling one row per component in place (x offset = out offset),
        // +-1; the row a whole number of 64 x 16 bytes with at most 32 components per lane.  (Whether the three rows ARE one row is
        // known when they are bound: run_reduce.)
        if (!(plan.flags & GAAST_FLAG_EXACT_ORDER) && p1.a == p1.b && xop == p1.a) {
            const size_t per_piece = 64 * (plan.dtype == GAAST_F32 ? 4 : 2);   // components a wave moves per 16-byte load
            const Step::Reduce& q = f.reduce;
            const size_t R = q.ent1.size();
            bool okw = R == q.ent2.size() && R % per_piece == 0 && (R / per_piece) * (per_piece / 64) <= 32 && q.coeff1.size() == R && q.coeff2.size() == R;
            const size_t pieces = okw ? R / per_piece : 0;
            okw = okw && (pieces == 1 || pieces == 2 || pieces == 4 || pieces == 8 || pieces == 16);
            std::vector<uint32_t> sg(128, 0u);
            std::vector<char> seen1(R, 0), seen2(R, 0);
            const size_t ec = per_piece / 64;
            auto place = [&](size_t c, int which) {   // component c of the row -> (lane, bit)
                const size_t piece = c / ec, e = c % ec, m = piece / 64, lane = piece % 64;
                sg[size_t(which) * 64 + lane] |= 1u << (m * ec + e);
            };
            for (size_t t = 0; okw && t < R; ++t) {
                const uint32_t li = q.ent1[t] & 0xffffu, ri = q.ent1[t] >> 16;
                okw = li == ri && li < R && !seen1[li] && (q.coeff1[t] == 1.0 || q.coeff1[t] == -1.0);
                if (okw) {
                    seen1[li] = 1;
                    if (q.coeff1[t] < 0) place(li, 0);
                }
            }
            for (size_t r = 0; okw && r < R; ++r) {
                const uint32_t xo = q.ent2[r] & 0xffffu, oo = q.ent2[r] >> 16;
                okw = xo == oo && xo < R && !seen2[xo] && (q.coeff2[r] == 1.0 || q.coeff2[r] == -1.0);
                if (okw) {
                    seen2[xo] = 1;
                    if (q.coeff2[r] < 0) place(xo, 1);
                }
            }
            if (okw) {
                f.reduce.wave = int(pieces);
                f.reduce.sign_words = std::move(sg);
            }
        }
        f.name = "reduce_scale[" + std::to_string(p1.list.entries.size()) + " comp-muls -> scalar" + (op == 1 ? ", 1/s" : op == 2 ? ", sqrt(s)" : "") + ", " +
                 std::to_string(p2.list.entries.size()) + " scaled components]";
        mark_dead(plan, S);
        plan.steps[i] = std::move(f);
        drop_steps(plan, i + 1, j + 1);
        return true;
    }
    return false;
}
static void fuse_reduce_scale(Plan& plan) {
    if (plan.flags & (GAAST_FLAG_NO_FUSION | GAAST_FLAG_DEBUG_NO_CHAIN)) return;
    while (fuse_one_reduce_scale(plan)) {}   // (indices move with every instance: look again from the start)
}

// A list with FEW LONG rows that stayed a launch of its own -- b * c projected on a low grade: (a + b * c).g(2) at n = 8 is 28 rows of 256
// terms -- gives k_product_ell (a thread per row) 28 busy threads per workgroup.  The specialised chain kernel's second list is exactly
// this shape (lane = (row, item), 32 items per workgroup): the list runs on it alone.  When the step before it is the covering copy of
// an input's grades into the same buffer (a + ...), that copy is folded in as well: the accumulators start from 0.0 + a -- ONE launch.
// Same order, same roundings; k_product_ell (and the copy) stay in charge when hiprtc is not available.
static void jit_long_row_lists(Plan& plan) {
    if (plan.flags & (GAAST_FLAG_NO_FUSION | GAAST_FLAG_NO_JIT | GAAST_FLAG_DEBUG_JIT_FAILS | GAAST_FLAG_DEBUG_NO_CHAIN)) return;
    for (size_t j = 0; j < plan.steps.size(); ++j) {
        Step& c = plan.steps[j];
        if (c.kind != Step::PRODUCT_CSR || c.list.ell_width < 32 || !c.list.ell_bytes || c.chain.side || c.cj.on) continue;
        const int64_t rows = int64_t(c.list.row_out.size());
        if (rows > 128 || c.a.idx < 0 || c.b.idx < 0) continue;
        const int64_t la = plan.layout(c.a).row_len, lb = plan.layout(c.b).row_len;
        // the covering copy right before it, into the same buffer?
        std::vector<uint32_t> init;
        bool fold = false;
        if (j > 0 && c.beta == 1) {
            const Step& ax = plan.steps[j - 1];
            if (ax.kind == Step::AXPY && ax.beta == 0 && ax.res == c.res && ax.a.kind == BufKind::INPUT && int64_t(ax.axpy_map.size()) == rows) {
                std::vector<int64_t> src_of(size_t(plan.layout(c.res).row_len), -1);
                for (uint32_t m : ax.axpy_map) src_of[m & 0xffffu] = int64_t(m >> 16);
                fold = true;
                for (int64_t r = 0; r < rows && fold; ++r) {
                    fold = src_of[c.list.row_out[size_t(r)]] >= 0;
                    init.push_back(uint32_t(fold ? src_of[c.list.row_out[size_t(r)]] : 0));
                }
            }
        }
        make_chain_jit(plan, c, nullptr, 0, 0, la, lb, 0, 1, true, fold ? &init : nullptr);
        if (!c.cj.on) continue;
        c.cj.single = 1;
        if (fold) {
            c.cj.fold_prev = 1;
            c.cj.init_src = plan.steps[j - 1].a;   // the copy's source: the accumulators' starting values
        }
    }
}

void run_plan_passes(Plan& plan) {
    fuse_elementwise_runs(plan);
    fuse_reduce_scale(plan);
    chain_sparse_into_dense(plan);
    uniform_csr_to_ell(plan);
    chain_list_into_list(plan);
    jit_long_row_lists(plan);
}

}  // namespace gaast
