// explog_adj_series.hip.hpp -- series thresholds and coefficients of the exp / log adjoints, shared by k_exp_log_adj
// (kernels_exact.hip.hpp) and the statements generated for gaast_jit (plan_fused.cpp).  Plain constexpr: host and device.
#pragma once

namespace gaast {

// The exp / log adjoints (Step::EXPLOG_ADJ) sum h = (c0 - f) / s (exp) and h = (a / D - f) / s (log) from their series where
// the quotient cancels; one definition for k_exp_log_adj and the statements generated for gaast_jit.
//   exp: h = sum_{n >= 1} 2n / (2n + 1)! s^(n-1) for |s| < 4 (the quotient amplifies the error of c0 and f by
//        (|c0| + |f|) / |c0 - f| <= 3 from there on); 14 terms in f64, 8 in f32: the first term left out is below eps / 8 of h;
//   log: h = a^-3 sum_{n >= 1} 2n / (2n + 1) u^(n-1), u = s / a^2, for |u| < 1/4 where the forward is analytic in s (a > 0, or
//        s > 0; and s == 0 itself, whose forward branch is 1 / a for either sign of a); 30 terms in f64, 14 in f32 (the series is
//        geometric: 4^-30 < eps / 100).  At the threshold the quotient amplifies by (|a / D| + |f|) / |a / D - f| <= 10.4.
constexpr double kExpAdjSeriesBelow = 4.0, kLogAdjSeriesBelow = 0.25;
constexpr int exp_adj_series_terms(bool f32) { return f32 ? 8 : 14; }
constexpr int log_adj_series_terms(bool f32) { return f32 ? 14 : 30; }
constexpr double exp_adj_series_coeff(int n) {   // 2n / (2n + 1)!
    double fact = 1.0;
    for (int i = 2; i <= 2 * n + 1; ++i) fact *= double(i);
    return 2.0 * double(n) / fact;
}
constexpr double log_adj_series_coeff(int n) { return 2.0 * double(n) / (2.0 * double(n) + 1.0); }

}  // namespace gaast
