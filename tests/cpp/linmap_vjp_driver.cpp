// Stand-alone check (own main, built with -fsanitize=address,undefined by tests/test_linmap_vjp_host.py) of the host side of the
// outermorphism's reverse mode with respect to its matrix (common/metric_basis.hpp): for n = 1 ... 8 and every grade k
//   - compound_vjp_terms lists every (I, J, i, j) with i in I, j in J exactly once, every index in range, the sign that of the
//     cofactor, the minor's index that of (I \ i, J \ j);
//   - compound_matrix_vjp (the sum over that list) equals the derivative of sum W . C_k(M) where it is easy to state exactly:
//     the directional derivative along M itself is k * sum W . C_k(M) (a k x k minor is homogeneous of degree k).
#include <cmath>
#include <cstdio>
#include <set>
#include <tuple>
#include <vector>

#include "metric_basis.hpp"

using namespace gaast;

static int fails = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            std::printf("FAIL %s: ", #cond);   \
            std::printf(__VA_ARGS__);          \
            std::printf("\n");                 \
            ++fails;                           \
        }                                      \
    } while (0)

int main() {
    uint64_t seed = 0x9e3779b97f4a7c15ULL;
    auto rnd = [&]() {
        seed = seed * 6364136223846793005ULL + 1442695040888963407ULL;
        return double(int64_t(seed >> 11) % 2000001 - 1000000) / 1000000.0;
    };
    for (int n = 1; n <= 8; ++n) {
        const BladeTable t(n);
        std::vector<double> m(size_t(n * n));
        for (double& v : m) v = rnd();
        for (int k = 0; k <= n; ++k) {
            std::vector<CompoundVjpTerm> terms;
            compound_vjp_terms(t, k, terms);
            const size_t d = t.grade_dim[size_t(k)], dp = k ? t.grade_dim[size_t(k - 1)] : 0;
            CHECK(terms.size() == (k ? d * d * size_t(k) * size_t(k) : 0), "n %d k %d: %zu terms", n, k, terms.size());
            std::set<std::tuple<uint32_t, uint32_t>> seen;
            for (const CompoundVjpTerm& e : terms) {
                CHECK(e.w < d * d && e.minor < dp * dp && e.target < n * n && e.negative <= 1, "n %d k %d: index out of range", n, k);
                if (e.w >= d * d || e.target >= n * n) continue;
                const uint32_t bi = t.blade_of[size_t(k)][e.w / d], bj = t.blade_of[size_t(k)][e.w % d];
                const int i = e.target / n, j = e.target % n;
                CHECK(((bi >> i) & 1u) && ((bj >> j) & 1u), "n %d k %d: target (%d, %d) outside its blades", n, k, i, j);
                CHECK(seen.insert(std::make_tuple(e.w, uint32_t(e.target))).second, "n %d k %d: (I, J, i, j) listed twice", n, k);
                const int pi = __builtin_popcount(bi & ((1u << i) - 1u)), pj = __builtin_popcount(bj & ((1u << j) - 1u));
                CHECK(e.negative == ((pi + pj) & 1), "n %d k %d: sign", n, k);
                CHECK(e.minor == t.index_of[bi & ~(1u << i)] * dp + t.index_of[bj & ~(1u << j)], "n %d k %d: minor index", n, k);
            }
            // every (I, J, i in I, j in J) is there: the count matches and none is listed twice
            CHECK(seen.size() == terms.size(), "n %d k %d: %zu distinct of %zu", n, k, seen.size(), terms.size());

            std::vector<double> w(d * d), dm(size_t(n * n), 0.0);
            for (double& v : w) v = rnd();
            compound_matrix_vjp(n, k, m.data(), w.data(), dm.data());
            std::vector<std::vector<double>> c;
            compound_matrices(n, m.data(), k, c);
            double lhs = 0.0, rhs = 0.0, mag = 0.0;
            for (int e = 0; e < n * n; ++e) lhs += dm[size_t(e)] * m[size_t(e)];
            for (size_t e = 0; e < d * d; ++e) {
                rhs += w[e] * c[size_t(k)][e];
                mag += std::fabs(w[e] * c[size_t(k)][e]);
            }
            rhs *= k;
            // Euler's identity <dM, M> = k L; each side is a sum of products of k + 1 factors in [-1, 1]: roundoff only
            CHECK(std::fabs(lhs - rhs) <= 1e-12 * (double(k) * mag + 1.0) * double(k * k + 1), "n %d k %d: <dM, M> = %.17g, k L = %.17g", n, k, lhs, rhs);
        }
    }
    if (fails) {
        std::printf("%d FAILED\n", fails);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
