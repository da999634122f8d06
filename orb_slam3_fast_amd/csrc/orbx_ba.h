// orbx_ba.h — the blocked dense LDLT of orbx_ba.hip: what the solver's kernels, the bundle adjustments' chain (orbx_lba.hip) and
// the C ABI (orbx_api_ba.hip) share.
#ifndef ORBX_BA_H
#define ORBX_BA_H
#include "orbx_host.h"

namespace orbx {

constexpr int kBaNB = 48;     // columns of a block column (a multiple of 6: a key frame's rows never straddle two)
constexpr int kBaTile = 64;   // rows of a panel tile, rows and columns of a trailing-update tile

// S x = bs for the symmetric positive definite n x n S.  S is row-major and is the factorisation's workspace (lower triangle:
// L below the diagonal, D on it; the upper triangle is not read); bs becomes z = D^-1 L^-1 bs and is then consumed by the
// back-substitution.  *ok is written by the chain: 1, or 0 when a pivot is <= 0 or not finite, and then x is not written.
struct BaSolveArgs {
  double* S;    // [n][n]
  double* bs;   // [n]
  double* x;    // [n]
  int* ok;
  int n;
};

// the whole chain on the null stream: 3 launches per block column and one more per block column for L^T x = z; n == 0 launches
// nothing and leaves *ok as it is
hipError_t launch_ba_solve(const BaSolveArgs& a);

}  // namespace orbx
#endif
