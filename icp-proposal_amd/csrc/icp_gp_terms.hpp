// icp_gp_terms.hpp — the scalar base kernels of a GP model's terms on the device, shared by kernels_gp_model.hip (pivoted Cholesky) and
// kernels_nystrom_model.hip (Nyström): the Gaussian and the cubic B-spline of include/icp_proposal.h.  One operation at a time (the
// units are built without contraction); the lattice indices are doubles, exact below 2^31.
#pragma once
#include "icp_kernels.hpp"

namespace icp {

__device__ __forceinline__ double gpm_beta3(double t) {
  const double a = fabs(t);
  if (a < 1.0) return (2.0 / 3.0 - a * a) + ((0.5 * a) * a) * a;
  if (a < 2.0) return (((1.0 / 6.0) * (2.0 - a)) * (2.0 - a)) * (2.0 - a);
  return 0.0;
}
// S(u, v) = Σ_k β(u − k)·β(v − k), k = ⌈max(u, v) − 2⌉ … ⌊min(u, v) + 2⌋ ascending: at most five k
__device__ __forceinline__ double gpm_spline_sum(double u, double v) {
  const double k0 = ceil(fmax(u, v) - 2.0), k1 = floor(fmin(u, v) + 2.0);
  double s = 0.0;
  for (double k = k0; k <= k1; k += 1.0) s = s + gpm_beta3(u - k) * gpm_beta3(v - k);
  return s;
}
// the scalar base kernel of a term between x and p
__device__ __forceinline__ double gpm_base(const GpmTerm& tm, double x0, double x1, double x2, double p0, double p1, double p2) {
  if (tm.kind == 0) {
    const double dx = x0 - p0, dy = x1 - p1, dz = x2 - p2;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    return exp(-(d2 / tm.sigma2));
  }
  const double c = tm.c;
  return (gpm_spline_sum(x0 * c, p0 * c) * gpm_spline_sum(x1 * c, p1 * c)) * gpm_spline_sum(x2 * c, p2 * c);
}

}  // namespace icp
