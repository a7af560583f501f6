// Constraint operators of the caller-side step before / after refinement
// (reference constraint.py:95-164): elementwise kernels.  The matrix inverse of
// ConstraintPropagation is composed from these and the fp64 MFMA GEMM in constraint_api.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "sc_internal.h"

namespace sc {

// ---- AffinityIntegration (constraint.py:106-118): max(A, Q) or 0.5 (A + Q) ------
__global__ __launch_bounds__(256) void k_affinity_integration(const double* __restrict__ a,
                                                              const double* __restrict__ q,
                                                              double* __restrict__ out, int n,
                                                              int ld, int type) {
  const int row = blockIdx.y;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= n) return;
  const size_t at = (size_t)row * ld + col;
  const double x = a[at], c = q[at];
  // np.maximum propagates NaN from either side; fmax would drop it
  out[at] = type == SC_INTEGRATION_MAX ? ((x != x || c != c) ? (x + c) : (x > c ? x : c))
                                       : 0.5 * (x + c);
}

// ---- the same against a banded Q (ConstraintMatrix.compute_diagonals, constraint.py:188-201):
// Q[i, i+1] = Q[i+1, i] = band[i], 0 elsewhere -- no constraint matrix is read
__global__ __launch_bounds__(256) void k_affinity_integration_band(
    const double* __restrict__ a, const double* __restrict__ band, double* __restrict__ out,
    int n, int ld, int type) {
  const int row = blockIdx.y;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= n) return;
  const size_t at = (size_t)row * ld + col;
  const double x = a[at];
  const double c = col == row + 1 ? band[row] : (row == col + 1 ? band[col] : 0.0);
  out[at] = type == SC_INTEGRATION_MAX ? ((x != x || c != c) ? (x + c) : (x > c ? x : c))
                                       : 0.5 * (x + c);
}

// ---- ConstraintPropagation, step 1 (constraint.py:143-152) ----------------------
// dn_i = 1 / (sqrt(deg_i) + EPS);  P = alpha * ((dn_i A_ij) dn_j);  T0 = I + P
// (first factor of the Neumann product).  Padding columns are zero-filled so the GEMMs
// may read whole 16-wide K tiles.
__device__ __forceinline__ void cp_prepare_body(const double* __restrict__ a,
                                                const double* __restrict__ deg, double alpha,
                                                double* __restrict__ p, double* __restrict__ t0,
                                                int n, int ld) {
  const int row = blockIdx.y;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= ld) return;
  const size_t at = (size_t)row * ld + col;
  if (col >= n) {
    p[at] = 0.0;
    t0[at] = 0.0;
    return;
  }
  const double di = 1.0 / (sqrt(deg[row]) + 1e-10);
  const double dj = 1.0 / (sqrt(deg[col]) + 1e-10);
  const double v = alpha * ((di * a[at]) * dj);
  p[at] = v;
  t0[at] = (row == col ? 1.0 : 0.0) + v;
}
__global__ __launch_bounds__(256) void k_cp_prepare(const double* __restrict__ a,
                                                    const double* __restrict__ deg,
                                                    double alpha, double* __restrict__ p,
                                                    double* __restrict__ t0, int n, int ld) {
  cp_prepare_body(a, deg, alpha, p, t0, n, ld);
}
// ... of every member of a group (blockIdx.z = member; CpItem: src = A, vec = deg, dst = P,
// dst2 = T0)
__global__ __launch_bounds__(256) void k_cp_prepare_g(const GroupOf<CpItem> g, double alpha) {
  const CpItem& m = g.s[blockIdx.z];
  if ((int)blockIdx.y >= m.n || (int)blockIdx.x * 256 >= m.ld) return;
  cp_prepare_body(m.src, m.vec, alpha, m.dst, m.dst2, m.n, m.ld);
}

// ---- ConstraintPropagation against a banded Q: X = Tt Q^T without the GEMM --------
// X[i, j] = band[j-1] Tt[i, j-1] + band[j] Tt[i, j+1]  (terms outside [0, n) dropped), the
// operand launch_gemm_nt(T, X) = T X^T = T Q T expects.  One read and one write of the matrix:
// a thread owns two adjacent columns (one 16-byte load and store; rows start on 128-byte
// lines and ld is even), the columns left and right of its pair come from the neighbouring
// lanes' registers, and only the first / last lane of a wavefront fetch theirs (a line the next
// wavefront loads anyway).  Padding columns [n, ld) are written as zero, as in k_cp_prepare.
__device__ __forceinline__ void cp_band_product_body(const double* __restrict__ tt,
                                                     const double* __restrict__ band,
                                                     double* __restrict__ x, int n, int ld) {
  const int row = blockIdx.y;
  const int j0 = (blockIdx.x * 256 + threadIdx.x) * 2;
  const bool live = j0 < ld;  // (no early return: every lane takes part in the shuffles)
  const double* r = tt + (size_t)row * ld;
  double2 v = make_double2(0.0, 0.0);
  if (live) v = *reinterpret_cast<const double2*>(r + j0);
  // band[j0] and band[j0 + 1]; an index outside [0, n - 1) marks a dropped term
  const bool has0 = j0 < n - 1, has1 = j0 + 1 < n - 1;
  const double b0 = has0 ? band[j0] : 0.0;
  const double b1 = has1 ? band[j0 + 1] : 0.0;
  double left = __shfl_up(v.y, 1);    // Tt[row, j0 - 1]
  double bm = __shfl_up(b1, 1);       // band[j0 - 1]
  double right = __shfl_down(v.x, 1);  // Tt[row, j0 + 2]
  const int lane = threadIdx.x & 63;
  const bool hasm = j0 >= 1 && j0 - 1 < n - 1;
  if (lane == 0 && hasm) {
    left = r[j0 - 1];
    bm = band[j0 - 1];
  }
  if (lane == 63 && has1) right = r[j0 + 2];
  if (!live) return;
  double2 o;
  o.x = j0 < n ? (hasm ? bm * left : 0.0) + (has0 ? b0 * v.y : 0.0) : 0.0;
  o.y = j0 + 1 < n ? (has0 ? b0 * v.x : 0.0) + (has1 ? b1 * right : 0.0) : 0.0;
  *reinterpret_cast<double2*>(x + (size_t)row * ld + j0) = o;
}
__global__ __launch_bounds__(256) void k_cp_band_product(const double* __restrict__ tt,
                                                         const double* __restrict__ band,
                                                         double* __restrict__ x, int n, int ld) {
  cp_band_product_body(tt, band, x, n, ld);
}
// (CpItem: src = Tt, vec = band, dst = X; whole workgroups leave, so every lane of a wavefront
// that stays takes part in the shuffles)
__global__ __launch_bounds__(256) void k_cp_band_product_g(const GroupOf<CpItem> g) {
  const CpItem& m = g.s[blockIdx.z];
  if ((int)blockIdx.y >= m.n || (int)blockIdx.x * 512 >= m.ld) return;
  cp_band_product_body(m.src, m.vec, m.dst, m.n, m.ld);
}

// ---- ConstraintPropagation, last step (constraint.py:153-163) -------------------
// F = (1 - alpha)^2 (T Q T);  F > 0: 1 - (1 - F)(1 - A);  else: (1 + F) A
__device__ __forceinline__ void cp_adjust_body(const double* __restrict__ tqt,
                                               const double* __restrict__ a, double scale,
                                               double* __restrict__ out, int n, int ld) {
  const int row = blockIdx.y;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= n) return;
  const size_t at = (size_t)row * ld + col;
  const double f = scale * tqt[at];
  const double x = a[at];
  // the reference evaluates both branches on masked operands and adds them; the
  // inactive branch contributes exactly 0 (1 - 1*1, or (1 + 0) * 0)
  out[at] = f > 0.0 ? (1.0 - (1.0 - f) * (1.0 - x)) + 0.0 : 0.0 + (1.0 + f) * x;
}
__global__ __launch_bounds__(256) void k_cp_adjust(const double* __restrict__ tqt,
                                                   const double* __restrict__ a, double scale,
                                                   double* __restrict__ out, int n, int ld) {
  cp_adjust_body(tqt, a, scale, out, n, ld);
}
// (CpItem: src = T Q T, vec = A, dst = the adjusted affinity -- may be A itself)
__global__ __launch_bounds__(256) void k_cp_adjust_g(const GroupOf<CpItem> g, double scale) {
  const CpItem& m = g.s[blockIdx.z];
  if ((int)blockIdx.y >= m.n || (int)blockIdx.x * 256 >= m.n) return;
  cp_adjust_body(m.src, m.vec, scale, m.dst, m.n, m.ld);
}

// ---- out = in^T (32x32 tiles through LDS), padding columns zeroed ----------------
__global__ __launch_bounds__(256) void k_transpose(const double* __restrict__ in,
                                                   double* __restrict__ out, int n, int ld) {
  __shared__ double tile[32][33];
  const int bi = blockIdx.y * 32, bj = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int r = ty; r < 32; r += 8) {
    const int gi = bj + r, gj = bi + tx;
    tile[r][tx] = (gi < n && gj < n) ? in[(size_t)gi * ld + gj] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int r = ty; r < 32; r += 8) {
    const int gi = bi + r, gj = bj + tx;
    if (gi < n && gj < ld) out[(size_t)gi * ld + gj] = gj < n ? tile[tx][r] : 0.0;
  }
}

// ---- 1 if in == in^T exactly (NaN counts as asymmetric), else 0, into *flag ------
__global__ __launch_bounds__(256) void k_symmetry_flag(const double* __restrict__ in, int n,
                                                       int ld, int* __restrict__ flag) {
  const int row = blockIdx.y;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= n || col <= row) return;
  if (!(in[(size_t)row * ld + col] == in[(size_t)col * ld + row])) *flag = 0;
}

void launch_affinity_integration(hipStream_t s, const double* a, const double* q, double* out,
                                 int n, int ld, int type) {
  hipLaunchKernelGGL(k_affinity_integration, dim3((n + 255) / 256, n), dim3(256), 0, s, a, q,
                     out, n, ld, type);
}
void launch_affinity_integration_band(hipStream_t s, const double* a, const double* band,
                                      double* out, int n, int ld, int type) {
  hipLaunchKernelGGL(k_affinity_integration_band, dim3((n + 255) / 256, n), dim3(256), 0, s, a,
                     band, out, n, ld, type);
}
void launch_cp_band_product(hipStream_t s, const double* tt, const double* band, double* x,
                            int n, int ld) {
  hipLaunchKernelGGL(k_cp_band_product, dim3((ld / 2 + 255) / 256, n), dim3(256), 0, s, tt, band,
                     x, n, ld);
}
void launch_cp_prepare(hipStream_t s, const double* a, const double* deg, double alpha,
                       double* p, double* t0, int n, int ld) {
  hipLaunchKernelGGL(k_cp_prepare, dim3((ld + 255) / 256, n), dim3(256), 0, s, a, deg, alpha,
                     p, t0, n, ld);
}
void launch_cp_adjust(hipStream_t s, const double* tqt, const double* a, double scale,
                      double* out, int n, int ld) {
  hipLaunchKernelGGL(k_cp_adjust, dim3((n + 255) / 256, n), dim3(256), 0, s, tqt, a, scale,
                     out, n, ld);
}
// grouped forms: one launch for up to kGroupMax members, blockIdx.z = member (n = 0: idle)
static GroupOf<CpItem> cp_pack(const CpItem* items, int count, int* nmax, int* ldmax) {
  GroupOf<CpItem> g;
  memset(&g, 0, sizeof(g));
  *nmax = *ldmax = 0;
  for (int z = 0; z < count && z < kGroupMax; ++z) {
    if (items[z].n <= 0) continue;
    g.s[z] = items[z];
    *nmax = std::max(*nmax, items[z].n);
    *ldmax = std::max(*ldmax, items[z].ld);
  }
  return g;
}
void launch_cp_prepare_group(hipStream_t s, const CpItem* items, int count, double alpha) {
  int nmax, ldmax;
  const GroupOf<CpItem> g = cp_pack(items, count, &nmax, &ldmax);
  if (nmax == 0) return;
  hipLaunchKernelGGL(k_cp_prepare_g, dim3((ldmax + 255) / 256, nmax, count), dim3(256), 0, s, g,
                     alpha);
}
void launch_cp_band_product_group(hipStream_t s, const CpItem* items, int count) {
  int nmax, ldmax;
  const GroupOf<CpItem> g = cp_pack(items, count, &nmax, &ldmax);
  if (nmax == 0) return;
  hipLaunchKernelGGL(k_cp_band_product_g, dim3((ldmax / 2 + 255) / 256, nmax, count), dim3(256), 0,
                     s, g);
}
void launch_cp_adjust_group(hipStream_t s, const CpItem* items, int count, double scale) {
  int nmax, ldmax;
  const GroupOf<CpItem> g = cp_pack(items, count, &nmax, &ldmax);
  if (nmax == 0) return;
  hipLaunchKernelGGL(k_cp_adjust_g, dim3((nmax + 255) / 256, nmax, count), dim3(256), 0, s, g,
                     scale);
}
void launch_transpose(hipStream_t s, const double* in, double* out, int n, int ld) {
  const int t = (n + 31) / 32, tc = (ld + 31) / 32;
  hipLaunchKernelGGL(k_transpose, dim3(tc, t), dim3(256), 0, s, in, out, n, ld);
}
void launch_symmetry_flag(hipStream_t s, const double* in, int n, int ld, int* flag) {
  hipLaunchKernelGGL(k_symmetry_flag, dim3((n + 255) / 256, n), dim3(256), 0, s, in, n, ld,
                     flag);
}

}  // namespace sc
