// The Dormand-Prince tableau and the Butcher-row -> Comb conversion: shared by the fused solver (solver.hip, which
// defines the tableau), the taped backward pass (api_backprop.hip) and the generic solver (api_flat.hip).
#pragma once
#include "node_internal.h"

#include <cstring>

namespace node {

extern const double DP_ALPHA[6];
extern const double DP_CMID[7];
extern const double DP_BETA[6][6];

// y + scale * sum_j coef_j k_j as the kernels take it: zero coefficients dropped
inline Comb make_comb(const float* y, float* const* k, const double* coef, int ncoef, int scale_mode) {
  Comb c;
  memset(&c, 0, sizeof(c));
  c.y = y;
  c.scale_mode = scale_mode;
  int nk = 0;
  for (int j = 0; j < ncoef; ++j) {
    if (coef[j] == 0.0) continue;
    c.k[nk] = k[j];
    c.coef[nk] = (float)coef[j];
    ++nk;
  }
  c.nk = nk;
  return c;
}

}  // namespace node
