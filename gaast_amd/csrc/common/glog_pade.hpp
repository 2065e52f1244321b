// glog_pade.hpp -- the [7/7] Pade approximant of log(1 + x) in partial fractions (GAAST_OP_GLOG, gaast_hip.h):
//   r_7(x) = sum_j alpha_j x / (1 + beta_j x),  alpha_j and beta_j the weights and nodes of 7-point Gauss-Legendre quadrature on [0, 1]
// (log(1 + x) = int_0^1 x / (1 + t x) dt).  The values are numpy.polynomial.legendre.leggauss(7) mapped to [0, 1], digit for digit
// (tests/test_glog_host.py compares them); its weights lie up to 34 ulp from the exact ones, which moves r_7 by less than
// 2e-15 |x|^2 (the weights still sum to 1 to the last bit), below one eps of the result at |x| <= 1/4.
// Included by host code (tests) and by the device kernels (kernels_glog.hip.hpp).
#pragma once

namespace gaast {

constexpr int kGlogPadeTerms = 7;
constexpr double kGlogPadeNode[kGlogPadeTerms] = {
    0.025446043828620757, 0.12923440720030277, 0.2970774243113014, 0.5, 0.7029225756886985, 0.8707655927996972, 0.9745539561713792,
};
constexpr double kGlogPadeWeight[kGlogPadeTerms] = {
    0.06474248308443532, 0.1398526957446383, 0.19091502525255916, 0.20897959183673448, 0.19091502525255916, 0.1398526957446383, 0.06474248308443532,
};
constexpr double kGlogTheta = 0.25;   // roots are taken while wmax * sum |X - e_0| exceeds this
constexpr int kGlogMaxRoots = 16;     // S: an item still beyond kGlogTheta after this many roots is a domain error

}  // namespace gaast
