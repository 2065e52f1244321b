// Lowering of a Product node onto the dense kernels (rewrite (3) of plan.cpp's header) and onto the opt-in matrix-representation
// kernels: which family takes the product, in which algebra and basis, and the tables of its PRODUCT_DENSE step.  Where a blade
// sits inside an operand image is dense_images.hip.hpp's statement, not this file's.
#include "plan_internal.hpp"
#include "spinor_basis.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>

namespace gaast {
namespace {

// A host that cannot name the product (the Rust shim: the grades_to_produce closure is opaque,
// base_types.rs:60-64) sends GAAST_PROD_EXPLICIT.  A list big enough to matter for the dense
// kernels is compared entry by entry with the geometric product's list for the same grade
// sets and metric; only an exact match (indices and coefficient bits) is treated as one.
bool is_geometric_list(const LowerState& st, const ProductOperands& po) {
    const gaast_node_desc& nd = po.nd;
    if (nd.product_kind == GAAST_PROD_GEOMETRIC) return true;
    if (nd.product_kind != GAAST_PROD_EXPLICIT || !nd.comp_muls) return false;
    const int n = st.d.vec_space_dim;
    if (n < 6 || double(nd.n_comp_muls) * 32.0 < double(uint64_t(1) << (2 * n))) return false;   // (4^(n-1) / 8: parity-pure products)
    auto contribs = iter_contribs(nd.minimal_grade_mask, Selection{GAAST_PROD_GEOMETRIC, nullptr, nullptr}, po.lmin, po.rmin);
    if (comp_mul_count(n, contribs) != nd.n_comp_muls) return false;
    uint64_t e = 0;
    bool same = true;
    for_each_comp_mul(st.bt, st.d.metric_diag, contribs, [&](const gaast_comp_mul& m) {
        if (same && std::memcmp(&m, &nd.comp_muls[e], sizeof(gaast_comp_mul)) != 0) same = false;
        ++e;
    });
    return same;
}

int parity_of(uint64_t mask) {   // 0: only even grades, 1: only odd grades, -1: mixed or empty
    const uint64_t EVEN = 0x5555555555555555ULL;
    if (!mask) return -1;
    if (!(mask & ~EVEN)) return 0;
    if (!(mask & EVEN)) return 1;
    return -1;
}

// Basis permutation that brings a diagonal metric into the shape the dense kernels want: position j of the
// permuted basis holds original vector perm[j]; positions [0, L) (the "lo" bits of a blade) hold vectors that
// square to +-1 (+1 first), never 0.  uniform: the four lo vectors must all square to the same sign (vector-FMA
// kernel: compile-time sign pattern).  The identity is kept whenever it already qualifies.
bool dense_basis_permutation(const DenseFrame& f, int L, bool uniform, std::vector<int>& perm) {
    const int n = f.n;
    std::vector<int> plus, minus;   // by the SIGN of the square: a general entry g is rescaled to g / |g| (blade_scale)
    for (int i = 0; i < n; ++i) {
        if (f.metric[size_t(i)] > 0.0) plus.push_back(i);
        if (f.metric[size_t(i)] < 0.0) minus.push_back(i);
    }
    std::vector<int> lo;
    if (uniform) {
        if (int(plus.size()) >= L) lo.assign(plus.begin(), plus.begin() + L);
        else if (int(minus.size()) >= L) lo.assign(minus.begin(), minus.begin() + L);
        else return false;
    } else {
        if (int(plus.size() + minus.size()) < L) return false;
        for (int i : plus) if (int(lo.size()) < L) lo.push_back(i);
        for (int i : minus) if (int(lo.size()) < L) lo.push_back(i);
    }
    std::sort(lo.begin(), lo.end());
    std::vector<char> is_lo(size_t(n), 0);
    for (int i : lo) is_lo[size_t(i)] = 1;
    perm = lo;
    for (int i = 0; i < n; ++i)
        if (!is_lo[size_t(i)]) perm.push_back(i);
    return true;
}

// General diagonal metric on the dense kernels.  e_i = r_i f_i with r_i = sqrt|g_i| (1 for a null vector) gives a basis
// whose metric is sign(g_i) in {+1, -1, 0}; a blade e_S = w_S f_S, w_S = prod_{i in S} r_i.  So
//     C_T = (1 / w_T) * sum_{S ^ U = T} s'(S, U) (w_S A_S) (w_U B_U),
// s' the sign-metric coefficient: w_S w_U / w_T = prod_{i in S & U} |g_i| is the reference's coefficient magnitude
// (algebra.rs:78-81).  The operands are multiplied by w while they are staged, the result by 1 / w_T when it is stored:
// three more roundings per term than the +-1 / 0 case (the factors themselves are rounded once, from long double).
// Used only when every w_S and 1 / w_S stays within 2^+-40 (f32) / 2^+-300 (f64) -- no overflow or gradual underflow
// introduced by the rescaling for operands of ordinary magnitude; otherwise the exact list kernels keep the product.
bool metric_is_unit(const DenseFrame& f) {
    for (double g : f.metric)
        if (g != 1.0 && g != -1.0 && g != 0.0) return false;
    return true;
}
bool dense_scales_ok(const LowerState& st, const DenseFrame& f) {
    const gaast_program_desc& d = st.d;
    long double up = 1.0L, down = 1.0L;
    for (double g : f.metric) {
        if (!(g == g) || g == 1.0 / 0.0 || g == -1.0 / 0.0) return false;
        if (g == 0.0) continue;
        const long double r = sqrtl(fabsl((long double)g));
        if (r > 1.0L) up *= r;
        else down *= r;
    }
    if (f.pivot >= 0) {   // the reduction's own factors are powers of 1 / g_p up to (n - 1) / 2, and g_p itself
        const long double gp = fabsl((long double)d.metric_diag[f.pivot]);
        const long double worst = powl(gp > 1.0L ? gp : 1.0L / gp, (long double)((d.vec_space_dim + 1) / 2));
        up *= worst;
        down /= worst;
    }
    if (metric_is_unit(f) && (f.pivot < 0 || fabs(d.metric_diag[f.pivot]) == 1.0)) return true;
    const long double lim = st.plan.dtype == GAAST_F32 ? 0x1p40L : 0x1p300L;
    return up <= lim && down >= 1.0L / lim;
}
long double blade_scale(const DenseFrame& f, uint32_t S) {   // w_S in the frame's algebra
    long double w = 1.0L;
    for (int i = 0; i < f.n; ++i)
        if (((S >> i) & 1u) && f.metric[size_t(i)] != 0.0) w *= sqrtl(fabsl((long double)f.metric[size_t(i)]));
    return w;
}

// Parity-pure operands (the reference only ever multiplies the entries it needs, specialize.rs:162-183; even x even --
// rotor composition, the second product of every sandwich -- needs a quarter of the 4^n table).  The even subalgebra
// Cl+ of Cl(n) is a Clifford algebra of dimension n - 1 on the generators f_i = e_i e_p (i != p, e_p any non-null basis
// vector): f_i f_j = -f_j f_i, f_i^2 = -g_i g_p.  An even blade e_E is a multiple of the f-blade on E \ {p},
//     e_E = c(E) f_{E \ p},   c(E) = sigma(E) (-g_p)^(-floor(|E \ p| / 2)),   sigma(E) = (-1)^#{i in E : i > p} if p in E, else 1
// and an odd multivector is (even) e_p:  A = A~ e_p,  A~_{S ^ p} = A_S tau(S) (p in S ? 1 : 1 / g_p),  tau(S) = (-1)^#{i in S : i > p}.
// With X^ = e_p X e_p^-1 (even X: the blades containing p change sign):
//     even x even: A B                      odd x even: (A~ B^) e_p
//     even x odd : (A B~) e_p               odd x odd : g_p A~ B~^
// Every case is ONE product of two elements of Cl(n - 1) -- 4^(n-1) multiply-adds -- with per-component factors on the
// way in and on the way out: exactly what the operand maps (position, negate bit, scale) and the result map carry.
bool parity_reduced_frame(const gaast_program_desc& d, uint64_t lmask, uint64_t rmask, DenseFrame& f) {
    const int n = d.vec_space_dim;
    const int lp = parity_of(lmask), rp = parity_of(rmask);
    if (lp < 0 || rp < 0 || n - 1 < 6) return false;
    int p = -1;
    for (int i = n - 1; i >= 0 && p < 0; --i)
        if (d.metric_diag[i] != 0.0) p = i;
    if (p < 0) return false;
    f.n = n - 1;
    f.metric.clear();
    for (int i = 0; i < n; ++i)
        if (i != p) f.metric.push_back(-d.metric_diag[i] * d.metric_diag[p] == 0.0 ? 0.0 : -d.metric_diag[i] * d.metric_diag[p]);
    f.pivot = p;
    f.lpar = lp;
    f.rpar = rp;
    return true;
}

// which dense kernel family (false: none), in which algebra (frame) and in which basis of it (perm)
bool dense_family_for(const LowerState& st, const DenseFrame& f, uint64_t n_comp_muls, std::vector<int>& perm, DenseFamily& fam) {
    const Plan& plan = st.plan;
    const int n = f.n;
    auto take = [&](DenseFamily x) { fam = x; return true; };
    if (n < 6 || n > 14) return false;  // small algebras: the exact kernel is HBM-bound anyway
    // A general diagonal metric (algebra.rs:148-165 multiplies by ANY base_vec_dot, :79-81) runs in the rescaled basis
    // f_i = e_i / sqrt|g_i|; it needs finite, well-scaled factors, else the list kernels keep the product
    if (!dense_scales_ok(st, f)) return false;
    if (double(n_comp_muls) * 8.0 < double(uint64_t(1) << (2 * n))) return false;  // the tiled kernels always do 4^n multiply-adds
    const bool mfma_ok = plan.dtype == GAAST_F32 && !(plan.flags & GAAST_FLAG_NO_MFMA);
    // matrix-core variants: f32, n >= 10 (32 result columns per wave, five lo vectors) / n = 8, 9 (lo = 4 bits)
    // (k_gp_mfma32p: +A, -A, +B, -B images; n = 14 does not fit and runs on k_gp_mfma32)
    if (mfma_ok && n >= 10 && dense_basis_permutation(f, 5, false, perm)) return take(n <= 13 ? DenseFamily::MFMA32P : DenseFamily::MFMA32);
    if (n == 14) return false;      // both operands of an item (128 KiB in f32) fit the LDS of the matrix-core kernel only
    if (mfma_ok && (n == 8 || n == 9) && dense_basis_permutation(f, 4, false, perm)) return take(DenseFamily::MFMA16X4);   // k_gp_mfma16x4<float>
    // f64 (the reference's value type), n = 8 ... 12: v_mfma_f64_16x16x4_f64, one item per workgroup
    if (plan.dtype == GAAST_F64 && !(plan.flags & GAAST_FLAG_NO_MFMA) && n >= 8 && n <= 12 &&
        dense_basis_permutation(f, 4, false, perm))
        return take(DenseFamily::MFMA16X4);
    // n = 7, both value types: one wave per item on the 16x16x4 instructions (lo = 3 bits: three non-null vectors)
    if (n == 7 && !(plan.flags & GAAST_FLAG_NO_MFMA) && dense_basis_permutation(f, 3, false, perm)) return take(DenseFamily::MFMA7);
    // n = 6, both value types: four 16x16x4 instructions per item, ANY +-1 / 0 metric in the basis as it stands (signs and
    // vanishing terms are slots of the operand images and bits of the accumulators: no lo vectors, no permutation)
    if (n == 6 && !(plan.flags & GAAST_FLAG_NO_MFMA) && dense_basis_permutation(f, 0, false, perm)) return take(DenseFamily::MFMA6);
    if (dense_basis_permutation(f, 4, true, perm)) return take(DenseFamily::VECTOR_FMA);
    return false;
}

// Blade of the program's algebra -> blade of the kernel's permuted frame basis, with a factor: the adjoint relabelling, the parity
// reduction, the basis permutation and the rescaling of a general metric, composed.  image value = component * factor, stored
// negated when `neg` (the factor's sign and the permutation's reordering sign); the tables carry |factor|.
struct FrameMap {
    struct Image {
        uint32_t blade;       // of the frame's permuted basis
        uint32_t neg;
        long double factor;
    };
    const DenseFrame& frame;
    const double* metric;     // the program's
    int n;                    // ... and its dimension
    int adj = 0;              // GAAST_PROD_ADJ_LEFT / GAAST_PROD_ADJ_RIGHT: the adjoint of a geometric product, else 0
    uint32_t adj_z = 0;       // ... the null vectors
    bool identity = true;     // the frame's basis is used as it stands
    std::vector<uint32_t> new_blade, blade_sign;

    // blade R of the frame's basis <-> blade R' of its permuted basis, f_R = sign(R) f'_R' (the parity of the
    // inversions of the new positions of R's vectors taken in ascending original order)
    FrameMap(const DenseFrame& f, const std::vector<int>& perm, const gaast_program_desc& d, int product_kind)
        : frame(f), metric(d.metric_diag), n(d.vec_space_dim), new_blade(size_t(1) << f.n), blade_sign(size_t(1) << f.n) {
        adj = product_kind >= GAAST_PROD_ADJ_LEFT ? (product_kind & ~7) : 0;
        for (int i = 0; adj && i < n; ++i)
            if (metric[i] == 0.0) adj_z |= 1u << i;
        const int n2 = frame.n;
        std::vector<int> inv(size_t(n2), 0);
        for (int j = 0; j < n2; ++j) {
            inv[size_t(perm[size_t(j)])] = j;
            identity = identity && perm[size_t(j)] == j;
        }
        for (uint32_t S = 0; S < (1u << n2); ++S) {
            uint32_t S2 = 0, par = 0;
            for (int p = 0; p < n2; ++p) {
                if (!((S >> p) & 1u)) continue;
                const int q = inv[size_t(p)];
                par ^= uint32_t(__builtin_popcount(S2 >> (q + 1))) & 1u;
                S2 |= 1u << q;
            }
            new_blade[S] = S2;
            blade_sign[S] = par;
        }
    }

    // adjoint products (GAAST_PROD_ADJ_*): ADJ_LEFT multiplies (cotangent, B), ADJ_RIGHT (A, cotangent), so the kernel's
    // operands are (child0, child1) or (child1, child0); the cotangent's blades and the result's are relabelled k -> k ^ Z
    // (Z: the null vectors), the other operand's component j is scaled by rev(j) mn(j) (-1)^R(Z, j) (left adjoint) or
    // (-1)^R(j, Z) (right adjoint), mn the product of the non-null squares (tools/proto/adjoint_dense.py)
    uint32_t adj_operand(uint32_t S, bool right, long double* f) const {
        *f = 1.0L;
        if (!adj) return S;
        if ((adj == GAAST_PROD_ADJ_LEFT) != right) return S ^ adj_z;   // the cotangent
        const int k = __builtin_popcount(S);
        int sign = (k * (k - 1) / 2) & 1;
        sign ^= adj == GAAST_PROD_ADJ_LEFT ? reorder_parity(adj_z, S) : reorder_parity(S, adj_z);
        long double m = 1.0L;
        for (int i = 0; i < n; ++i)
            if (((S >> i) & 1u) && metric[i] != 0.0) m *= (long double)metric[i];
        *f = sign ? -m : m;
        return S;
    }

    // ---- the parity reduction (parity_reduced_frame): blade of the program's algebra -> blade of the frame's algebra, with a factor ----
    bool reduced() const { return frame.pivot >= 0; }
    long double gp() const { return (long double)metric[frame.pivot]; }
    bool has_p(uint32_t S) const { return ((S >> frame.pivot) & 1u) != 0; }
    long double tau(uint32_t S) const { return (__builtin_popcount(S >> (frame.pivot + 1)) & 1) ? -1.0L : 1.0L; }
    uint32_t compress(uint32_t E) const {   // drop bit p
        const int pv = frame.pivot;
        E &= ~(1u << pv);
        return (E & ((1u << pv) - 1u)) | ((E >> (pv + 1)) << pv);
    }
    long double c_of(uint32_t E) const {    // e_E = c(E) f_{E \ p} for an even blade E
        const int k = __builtin_popcount(E & ~(1u << frame.pivot));
        long double v = powl(-1.0L / gp(), (long double)(k / 2));
        return has_p(E) ? v * tau(E) : v;
    }
    long double t_of(uint32_t S) const { return tau(S) * (has_p(S) ? 1.0L : 1.0L / gp()); }   // odd S: A~_{S ^ p} = A_S t(S)
    // operand component on blade S -> (frame blade R, factor): image value = A_S * factor
    uint32_t operand_to_frame(uint32_t S, bool right, long double* factor) const {
        if (!reduced()) {
            *factor = 1.0L;
            return S;
        }
        const int par = right ? frame.rpar : frame.lpar;
        const uint32_t E = par ? S ^ (1u << frame.pivot) : S;
        long double f = (par ? t_of(S) : 1.0L) * c_of(E);
        if (right && frame.lpar == 1 && has_p(E)) f = -f;   // the conjugation e_p X e_p^-1 of the right operand
        *factor = f;
        return compress(E);
    }
    // result component on blade T <- (frame blade R, factor): C_T = C'_R * factor
    uint32_t result_from_frame(uint32_t T, long double* factor) const {
        if (!reduced()) {
            *factor = 1.0L;
            return T;
        }
        if ((frame.lpar ^ frame.rpar) == 0) {
            *factor = ((frame.lpar == 1) ? gp() : 1.0L) / c_of(T);
            return compress(T);
        }
        const uint32_t E = T ^ (1u << frame.pivot);   // C = P e_p: C_{E ^ p} = P_E tau(E) (p in E ? g_p : 1)
        *factor = tau(E) * (has_p(E) ? gp() : 1.0L) / c_of(E);
        return compress(E);
    }

    Image operand(uint32_t S, bool right) const {   // the component on blade S of the kernel's left / right operand
        long double fa, f1;
        const uint32_t orig = adj_operand(S, right, &fa);
        const uint32_t R = operand_to_frame(orig, right, &f1);
        const long double factor = fa * f1 * blade_scale(frame, R);
        return {new_blade[R], blade_sign[R] ^ (factor < 0.0L ? 1u : 0u), factor};
    }
    Image result(uint32_t T) const {                // the result component on blade T: C_T = C'_blade * factor
        long double f1;
        const uint32_t R = result_from_frame(adj ? (T ^ adj_z) : T, &f1);
        const long double factor = f1 / blade_scale(frame, R);
        return {new_blade[R], blade_sign[R] ^ (factor < 0.0L ? 1u : 0u), factor};
    }
};

// k_gp_mfma6: lane q moves the component of entry q into its four image slots; full operands are dealt to lanes by LDS bank
// (dense_images::mfma6_lane_of, with the bank-conflict figures)
void deal_mfma6_by_lane(std::vector<uint32_t>& map, std::vector<double>& scale, bool right, bool f32) {
    std::vector<uint32_t> m2(map.size());
    std::vector<double> s2(scale.size());
    for (size_t e = 0; e < map.size(); ++e) {
        const uint32_t q = dense_images::mfma6_lane_of((map[e] >> 16) & 63u, right, f32);
        m2[q] = map[e];
        s2[q] = scale[e];
    }
    map.swap(m2);
    scale.swap(s2);
}

// k_gp_mfma7 moves ONE component per lane and load (entry q = load * 64 + lane), so the entries can be dealt
// to lanes by LDS bank: the lanes that share an LDS cycle of a store (f32: 32 lanes, bank = position mod 32;
// f64: 16 lanes of 8 bytes, position mod 16) get components of different banks -- every residue holds
// 128 / G positions of an image, one per run of G entries.  (Row order put 36 conflict cycles into the
// ~108 LDS cycles an item cost.)  The row offsets are no longer 0, 1, 2, ...: no 16-byte vector path.
bool deal_mfma7_by_bank(std::vector<uint32_t>& map, std::vector<double>& scale, bool f32) {   // false: the residues are uneven, row order stays
    const uint32_t G = f32 ? 32u : 16u;
    std::vector<std::vector<size_t>> bucket(G);
    for (size_t e = 0; e < map.size(); ++e) bucket[((map[e] >> 16) & 0x7fffu) % G].push_back(e);
    for (const auto& b : bucket)
        if (b.size() != map.size() / G) return false;
    std::vector<uint32_t> m2;
    std::vector<double> s2;
    for (size_t r = 0; r < map.size() / G; ++r)
        for (uint32_t k = 0; k < G; ++k) {
            m2.push_back(map[bucket[k][r]]);
            s2.push_back(scale[bucket[k][r]]);
        }
    map.swap(m2);
    scale.swap(s2);
    return true;
}

// which operand of which kernel an operand map is built for
struct ImageKind {
    DenseFamily family;
    bool right;         // the B image
    bool quads;         // k_gp_mfma16x4<float>: B words in 16-byte quads
    bool quad_planes;   // k_gp_mfma32p<false, 12, *, *>: the quad-plane B image
    bool f32;
};
// position of blade m of the permuted basis in the image the kernel reads: the one `case` a kernel family has here
uint32_t image_position(const ImageKind& k, uint32_t blade) {
    namespace di = dense_images;
    switch (k.family) {
    case DenseFamily::MFMA16X4: return !k.right ? blade : k.quads ? di::mfma16q_b_pos(blade) : di::mfma16d_b_pos(blade);
    case DenseFamily::MFMA32P: return !k.right ? blade : k.quad_planes ? b_planes::pos(blade) : di::mfma32p_b_pos(blade);
    case DenseFamily::MFMA32: return k.right ? di::mfma32_b_pos(blade) : blade;
    case DenseFamily::MFMA7: return k.right ? di::mfma7_b_pos(blade) : di::mfma7_a_pos(blade);
    case DenseFamily::MFMA6: return blade;   // k_gp_mfma6 derives its image slots from the blade itself
    default: return di::vec_pos(blade);
    }
}

// entry: row offset | image position << 16 | (negate while staging) << 31; scale[entry] = |factor| (when any != 1)
void build_operand_map(const LowerState& st, const FrameMap& fm, const ImageKind& kind, const Layout& lay, uint64_t want, uint64_t flip,
                       std::vector<uint32_t>& map, std::vector<double>& scale, int* full, int* contig) {
    bool seq = true;
    for (int k = 0; k <= fm.n; ++k) {
        if (!((want >> k) & 1ULL)) continue;
        for (uint32_t i = 0; i < st.bt.grade_dim[size_t(k)]; ++i) {
            const FrameMap::Image im = fm.operand(st.bt.blade_of[size_t(k)][i], kind.right);
            uint32_t neg = uint32_t((flip >> k) & 1ULL) ^ im.neg;
            if (kind.right) neg ^= dense_images::b_image_sign(kind.family, im.blade);
            const uint32_t sgn = neg ? 0x80000000u : 0u;
            const uint32_t off = uint32_t(lay.offset(k) + i);
            seq = seq && off == map.size();
            map.push_back(off | (image_position(kind, im.blade) << 16) | sgn);
            scale.push_back(double(fabsl(im.factor)));
        }
    }
    *full = map.size() == (size_t(1) << fm.frame.n);
    *contig = seq && map.size() % 4 == 0 && !map.empty();
    if (kind.family == DenseFamily::MFMA6 && *full) {
        deal_mfma6_by_lane(map, scale, kind.right, kind.f32);
        *contig = 0;
    }
    if (kind.family == DenseFamily::MFMA7 && *full && deal_mfma7_by_bank(map, scale, kind.f32)) *contig = 0;
}

// out_map: indexed by the blade of the frame's permuted basis; offset | sign << 30, or -1; out_scale: |factor|
void build_out_map(const LowerState& st, const FrameMap& fm, const Layout& lr, uint64_t prod_mask, Step::Dense& ds) {
    const int n2 = fm.frame.n;
    ds.out_map.assign(size_t(1) << n2, -1);
    ds.out_scale.assign(size_t(1) << n2, 1.0);
    for (uint32_t m = 0; m < (1u << fm.n); ++m) {
        const int g = __builtin_popcount(m);
        if (!((prod_mask >> g) & 1ULL)) continue;
        const FrameMap::Image im = fm.result(m);
        ds.out_map[im.blade] = int32_t(uint32_t(lr.offset(g) + st.bt.index_of[m]) | (im.neg << 30));
        ds.out_scale[im.blade] = double(fabsl(im.factor));
    }
    // scale tables only when some factor is not 1 (a general metric): +-1 / 0 metrics keep the register-prefetch paths
    ds.scaled = 0;
    for (const std::vector<double>* v : {&ds.left_scale, &ds.right_scale, &ds.out_scale})
        for (double x : *v) ds.scaled |= int(x != 1.0);
    if (!ds.scaled) {
        ds.left_scale.clear();
        ds.right_scale.clear();
        ds.out_scale.clear();
    }
    // every blade produced into a row that holds nothing else: whole rows can be written in 16-byte pieces
    ds.out_full = lr.row_len == (int64_t(1) << n2);
    for (uint32_t m = 0; m < (1u << n2); ++m) ds.out_full = ds.out_full && ds.out_map[m] >= 0;
    for (uint32_t w : ds.left_map) ds.left_signs |= int(w >> 31);
    for (uint32_t w : ds.right_map) ds.right_signs |= int(w >> 31);
    for (int32_t w : ds.out_map) ds.out_signs |= int(w >= 0 && (uint32_t(w) & 0x40000000u));
    ds.out_all = 1;
    for (int32_t w : ds.out_map) ds.out_all = ds.out_all && w >= 0;
}

// the metric of the permuted basis as the kernels take it: sign bits of the lo vectors, sign and null bits of the hi vectors
void fill_metric_bits(const DenseChoice& c, Step::Dense& ds) {
    const int lo_bits = dense_images::lo_bits(c.family);
    for (int j = 0; j < c.frame.n; ++j) {
        const double g = c.frame.metric[size_t(c.perm[size_t(j)])];   // only its sign matters here: the magnitude is in the scales
        if (j < lo_bits) {
            if (g < 0.0) ds.neg_lo |= 1u << j;
        } else {
            if (g < 0.0) ds.neg_hi |= 1u << (j - lo_bits);
            if (g == 0.0) ds.zero_hi |= 1u << (j - lo_bits);
        }
    }
    ds.neg_lo_all = c.family == DenseFamily::VECTOR_FMA && ds.neg_lo == 15u;
    ds.degenerate = ds.zero_hi != 0;
}

// blade -> Pauli string i^k X^x Z^z under the Jordan-Wigner generators (kernels_spinor.hip.hpp);
// vectors beyond the algebra's dimension (odd n padded to n + 1) square to +1
void pauli_string(const gaast_program_desc& d, uint32_t blade, uint32_t* x, uint32_t* z, uint32_t* k) {
    uint32_t px = 0, pz = 0, pk = 0;
    for (int v = 0; v < 32 && (blade >> v); ++v) {
        if (!((blade >> v) & 1u)) continue;
        const int j = v >> 1;
        const uint32_t gx = 1u << j;
        const uint32_t gz = (v & 1) ? (1u << (j + 1)) - 1u : (1u << j) - 1u;
        const bool negative = v < d.vec_space_dim && d.metric_diag[v] < 0.0;
        const uint32_t gk = uint32_t(v & 1) + (negative ? 1u : 0u);
        pk = (pk + gk + 2u * uint32_t(__builtin_popcount(pz & gx))) & 3u;
        px ^= gx;
        pz ^= gz;
    }
    *x = px;
    *z = pz;
    *k = pk;
}

// One table of the matrix-representation kernels: D*D 16-bit entries indexed by row offset, two per word (format: SpinorArgs).
// operands (role 0 left, 1 right): bit 0 = negate, bits [14:2] = x'*LD + z'; result (role 2): bit 0 = negate, bit 1 = nothing
// to store, bits [15:2] = x'*LD + z'
void build_spinor_map(const LowerState& st, const SpinorBasis& sb, int m, const Layout& lay, uint64_t want, uint64_t flip, int role,
                      std::vector<uint32_t>& packed, int* full) {
    const int n = st.d.vec_space_dim;
    const uint32_t D = 1u << m, LD = D + 1u;
    const uint16_t nothing = role == 2 ? uint16_t(2u) : uint16_t(D << 2);
    std::vector<uint16_t> map(size_t(D) * D, nothing);
    size_t count = 0;
    for (int k = 0; k <= n; ++k) {
        if (!((want >> k) & 1ULL)) continue;
        for (uint32_t i = 0; i < st.bt.grade_dim[size_t(k)]; ++i) {
            uint32_t px, pz, pk;
            pauli_string(st.d, st.bt.blade_of[size_t(k)][i], &px, &pz, &pk);
            const uint32_t x2 = sb.map_x(px), z2 = sb.map_z(pz);
            const uint32_t f = (sb.has_alpha ? (x2 >> (m - 1)) & 1u : 0u) ^
                               (sb.lam_bit >= 0 ? (z2 >> sb.lam_bit) & 1u : 0u);
            if (f != (pk & 1u)) throw std::runtime_error("spinor basis: phase parity mismatch");
            uint32_t neg = uint32_t((flip >> k) & 1ULL) ^ (pk >> 1);
            if (role != 0) neg ^= uint32_t(__builtin_popcount(x2 & z2) & 1);
            map[size_t(lay.offset(k) + i)] = uint16_t((x2 * LD + z2) << 2 | neg);
            ++count;
        }
    }
    *full = count == size_t(D) * D;
    packed.resize(map.size() / 2);
    std::memcpy(packed.data(), map.data(), map.size() * sizeof(uint16_t));
}

}  // namespace

bool dense_choice(const LowerState& st, const ProductOperands& po, DenseChoice& c) {
    const gaast_program_desc& d = st.d;
    const gaast_node_desc& nd = po.nd;
    if (st.plan.flags & (GAAST_FLAG_EXACT_ORDER | GAAST_FLAG_NO_FUSION)) return false;
    const int n = d.vec_space_dim;
    if (n < 6 || n > 15) return false;
    if (st.layout(po.res).dim != n || st.layout(po.l).dim != n || st.layout(po.r).dim != n) return false;
    if (nd.product_kind >= GAAST_PROD_ADJ_LEFT) {
        // adjoint of a geometric product: a forward product in the metric m' (1 / m off the null
        // vectors, 0 on them) of relabelled / re-signed / rescaled operands, always in the full frame
        if ((nd.product_kind & 7) != GAAST_PROD_GEOMETRIC || n > 14) return false;
        DenseFrame f;
        f.n = n;
        for (int i = 0; i < n; ++i) f.metric.push_back(d.metric_diag[i] == 0.0 ? 0.0 : 1.0 / d.metric_diag[i]);
        const bool found = dense_family_for(st, f, nd.n_comp_muls, c.perm, c.family);
        if (found) c.frame = f;
        return found;
    }
    const uint64_t lmask = po.lmin & st.layout(po.l).mask, rmask = po.rmin & st.layout(po.r).mask;
    bool geometric_known = false, geometric = false;
    auto is_gp = [&]() {
        if (!geometric_known) {
            geometric = is_geometric_list(st, po);
            geometric_known = true;
        }
        return geometric;
    };
    DenseFrame reduced;
    if (parity_reduced_frame(d, lmask, rmask, reduced) && dense_family_for(st, reduced, nd.n_comp_muls, c.perm, c.family) && is_gp()) {
        c.frame = reduced;
        return true;
    }
    DenseFrame full;
    full.n = n;
    full.metric.assign(d.metric_diag, d.metric_diag + n);
    if (n <= 14 && dense_family_for(st, full, nd.n_comp_muls, c.perm, c.family) && is_gp()) {
        c.frame = full;
        return true;
    }
    return false;
}

// opt-in matrix-representation kernels: f32, n = 7..12 (odd n as the subalgebra of n + 1), every
// vector squaring to +-1
bool spinor_eligible(const LowerState& st, const ProductOperands& po) {
    const gaast_program_desc& d = st.d;
    if (!(st.plan.flags & GAAST_FLAG_SPINOR_GEMM)) return false;
    if (st.plan.flags & (GAAST_FLAG_EXACT_ORDER | GAAST_FLAG_NO_FUSION)) return false;
    const int n = d.vec_space_dim;
    if (n < 7 || n > 12) return false;
    if (st.layout(po.res).dim != n || st.layout(po.l).dim != n || st.layout(po.r).dim != n) return false;
    for (int i = 0; i < n; ++i)
        if (d.metric_diag[i] != 1.0 && d.metric_diag[i] != -1.0) return false;
    if (!is_geometric_list(st, po)) return false;
    return double(po.nd.n_comp_muls) * 8.0 >= double(uint64_t(1) << (2 * n));
}

void lower_product_spinor(LowerState& st, const ProductOperands& po) {
    const Layout &lr = st.layout(po.res), &ll = st.layout(po.l), &lrr = st.layout(po.r);
    const uint64_t omin = po.nd.minimal_grade_mask;
    const bool beta0 = po.fresh_zero >= 0 && (lr.mask & ~omin) == 0;
    if (beta0) st.removed[size_t(po.fresh_zero)] = 1;
    const int n = st.d.vec_space_dim;
    const int m = (n + 1) / 2;                 // 2^m x 2^m complex matrices
    Step& s = st.emit(Step::PRODUCT_DENSE, po.res, "product_spinor_gemm[gp n=" + std::to_string(n) + "]");
    s.a = po.l;
    s.b = po.r;
    s.canon_a = po.canon_l;
    s.canon_b = po.canon_r;
    s.beta = beta0 ? 0 : 1;
    s.n_entries = po.nd.n_comp_muls;
    s.dense.family = DenseFamily::SPINOR;
    s.dense.spinor_m = m;
    // one real plane per operand: indices in the basis of spinor_basis.hpp
    uint32_t alpha = 0, lam = 0;
    for (uint32_t blade = 0; blade < (1u << (2 * m)); ++blade) {
        uint32_t px, pz, pk;
        pauli_string(st.d, blade, &px, &pz, &pk);
        if (pz == 0 && __builtin_popcount(px) == 1 && (pk & 1u)) alpha |= px;
        if (px == 0 && __builtin_popcount(pz) == 1 && (pk & 1u)) lam |= pz;
    }
    const SpinorBasis sb = choose_spinor_basis(m, alpha, lam);
    s.dense.spinor_lam_bit = sb.lam_bit;
    s.dense.spinor_has_alpha = sb.has_alpha ? 1 : 0;
    build_spinor_map(st, sb, m, ll, po.lmin & ll.mask, po.flip_l, 0, s.dense.left_map, &s.dense.left_full);
    build_spinor_map(st, sb, m, lrr, po.rmin & lrr.mask, po.flip_r, 1, s.dense.right_map, &s.dense.right_full);
    build_spinor_map(st, sb, m, lr, omin, 0, 2, s.dense.spinor_out_map, &s.dense.out_full);
    s.name = "product_spinor_gemm[gp n=" + std::to_string(n) + " lam=" + std::to_string(sb.lam_bit) + "]";
    st.touch(po.res);
}

void lower_product_dense(LowerState& st, const ProductOperands& po, const DenseChoice& c) {
    const gaast_node_desc& nd = po.nd;
    const Layout &lr = st.layout(po.res), &ll = st.layout(po.l), &lrr = st.layout(po.r);
    const DenseFrame& frame = c.frame;
    const DenseFamily fam = c.family;
    const int n = st.d.vec_space_dim;   // the program's algebra: graded rows, blade <-> (grade, index)
    const int n2 = frame.n;             // the kernel's algebra: n, or n - 1 for parity-pure operands
    const bool reduced = frame.pivot >= 0;
    // grades this step produces: a parity-pure product fills only the grades of its own parity
    uint64_t prod_mask = nd.minimal_grade_mask;
    if (reduced) prod_mask &= ((frame.lpar ^ frame.rpar) ? 0xAAAAAAAAAAAAAAAAULL : 0x5555555555555555ULL);
    const bool beta0 = po.fresh_zero >= 0 && (lr.mask & ~prod_mask) == 0;
    if (beta0) st.removed[size_t(po.fresh_zero)] = 1;
    const FrameMap fm(frame, c.perm, st.d, nd.product_kind);
    // the kernel's operands: (child0, child1), or (child1, child0) for a right adjoint (FrameMap::adj_operand)
    const bool swap_ops = fm.adj == GAAST_PROD_ADJ_RIGHT;
    const Layout &kla = swap_ops ? lrr : ll, &klb = swap_ops ? ll : lrr;
    const uint64_t kfa = swap_ops ? po.flip_r : po.flip_l, kfb = swap_ops ? po.flip_l : po.flip_r;
    const uint64_t kwa = swap_ops ? (po.rmin & lrr.mask) : (po.lmin & ll.mask), kwb = swap_ops ? (po.lmin & ll.mask) : (po.rmin & lrr.mask);
    Step& s = st.emit(Step::PRODUCT_DENSE, po.res, "product_dense[gp n=" + std::to_string(n) + "]");
    s.a = swap_ops ? po.r : po.l;
    s.b = swap_ops ? po.l : po.r;
    s.canon_a = swap_ops ? po.canon_r : po.canon_l;
    s.canon_b = swap_ops ? po.canon_l : po.canon_r;
    s.beta = beta0 ? 0 : 1;
    s.n_entries = nd.n_comp_muls;
    Step::Dense& ds = s.dense;   // (no step is emitted below: the reference stays valid)
    ds.n = n2;
    ds.family = fam;
    const bool f32 = st.plan.dtype == GAAST_F32;
    ds.mfma16_quads = fam == DenseFamily::MFMA16X4 && f32;   // k_gp_mfma16x4<float>: B words in 16-byte quads
    // k_gp_mfma32p at n = 12 with no null vector among the hi vectors -- the instantiations <false, 12, *, *>, whose step loop keeps
    // live B addresses: the quad-plane image of mfma32p_b_planes.hip.hpp instead of the block image
    bool b_quad_planes = fam == DenseFamily::MFMA32P && n2 == b_planes::kDim;
    for (int j = 5; j < n2; ++j) b_quad_planes = b_quad_planes && frame.metric[size_t(c.perm[size_t(j)])] != 0.0;
    build_operand_map(st, fm, ImageKind{fam, false, false, false, f32}, kla, kwa, kfa, ds.left_map, ds.left_scale, &ds.left_full, &ds.left_contig);
    build_operand_map(st, fm, ImageKind{fam, true, ds.mfma16_quads != 0, b_quad_planes, f32}, klb, kwb, kfb, ds.right_map, ds.right_scale, &ds.right_full,
                      &ds.right_contig);
    build_out_map(st, fm, lr, prod_mask, ds);
    fill_metric_bits(c, ds);
    if (b_quad_planes != (fam == DenseFamily::MFMA32P && n2 == b_planes::kDim && !ds.degenerate)) {   // the launcher picks the kernel by ds.degenerate
        st.fail(GAAST_ERR_INVALID_PROGRAM, "B image layout and kernel instantiation disagree");
        return;
    }
    static const char* const par_name[2] = {"even", "odd"};
    s.name = std::string(fam == DenseFamily::VECTOR_FMA ? "product_dense" : "product_dense_mfma") + "[gp n=" + std::to_string(n) +
             (reduced ? std::string(" ") + par_name[frame.lpar] + " x " + par_name[frame.rpar] + " in Cl(" + std::to_string(n2) + ")" : std::string()) +
             (fm.identity ? "" : " permuted basis") + (ds.scaled ? " rescaled basis" : "") +
             (fm.adj == GAAST_PROD_ADJ_LEFT ? " adjoint left" : fm.adj ? " adjoint right" : "") + "]";
    st.touch(po.res);
}

}  // namespace gaast
