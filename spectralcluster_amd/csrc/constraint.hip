// Constraint operators of the caller-side step before / after refinement
// (reference constraint.py:95-164): elementwise kernels.  The matrix inverse of
// ConstraintPropagation is composed from these and the fp64 MFMA GEMM in constraint_api.hip.
// A constraint given as K directed entries (sc_set_constraint_pairs) has kernels of its own:
// AffinityIntegration patches K elements, ConstraintPropagation forms T Q T as a rank-K product
// inside the kernel that adjusts the affinity (k_cp_pair_panels, k_cp_pairs_adjust).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "sc_internal.h"

namespace sc {

// ---- AffinityIntegration (constraint.py:106-118): max(A, Q) or 0.5 (A + Q) ------
// one element; np.maximum propagates NaN from either side, fmax would drop it
__device__ __forceinline__ double integrate_value(double x, double c, int type) {
  return type == SC_INTEGRATION_MAX ? ((x != x || c != c) ? (x + c) : (x > c ? x : c))
                                    : 0.5 * (x + c);
}
__global__ __launch_bounds__(256) void k_affinity_integration(const double* __restrict__ a,
                                                              const double* __restrict__ q,
                                                              double* __restrict__ out, int n,
                                                              int ld, int type) {
  const int row = blockIdx.y;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= n) return;
  const size_t at = (size_t)row * ld + col;
  out[at] = integrate_value(a[at], q[at], type);
}

// ---- the same against a Q given as k directed entries Q[rows[e], cols[e]] = vals[e], no two at
// one position (sc_set_constraint_pairs): the entries' original A first (out may alias a), one
// pass with Q = 0, then the k entries from the originals -- three launches on one stream
__global__ __launch_bounds__(256) void k_affinity_integration_pairs_gather(
    const double* __restrict__ a, const int32_t* __restrict__ rows,
    const int32_t* __restrict__ cols, int k, int ld, double* __restrict__ orig) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < k) orig[e] = a[(size_t)rows[e] * ld + cols[e]];
}
// (no __restrict__ on a / out: they may be one matrix; each element is read and written by
// the same lane)
__global__ __launch_bounds__(256) void k_affinity_integration_pairs(const double* a, double* out,
                                                                    int n, int ld, int type) {
  const int row = blockIdx.y;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= n) return;
  const size_t at = (size_t)row * ld + col;
  out[at] = integrate_value(a[at], 0.0, type);
}
__global__ __launch_bounds__(256) void k_affinity_integration_pairs_patch(
    const double* __restrict__ orig, const int32_t* __restrict__ rows,
    const int32_t* __restrict__ cols, const double* __restrict__ vals, int k, int ld, int type,
    double* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < k) out[(size_t)rows[e] * ld + cols[e]] = integrate_value(orig[e], vals[e], type);
}

// ---- the entries scattered into a zero-filled (n, ld) matrix: the dense Q of a list with more
// than n entries, without an (n, n) upload
__global__ __launch_bounds__(256) void k_pairs_to_dense(const int32_t* __restrict__ rows,
                                                        const int32_t* __restrict__ cols,
                                                        const double* __restrict__ vals, int k,
                                                        int ld, double* __restrict__ q) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < k) q[(size_t)rows[e] * ld + cols[e]] = vals[e];
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
  const double c = col == row + 1 ? band[row] : (row == col + 1 ? band[col] : 0.0);
  out[at] = integrate_value(a[at], c, type);
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
// one element: tqt = (T Q T)[i, j], x = A[i, j]
__device__ __forceinline__ double cp_adjust_value(double tqt, double x, double scale) {
  const double f = scale * tqt;
  // the reference evaluates both branches on masked operands and adds them; the
  // inactive branch contributes exactly 0 (1 - 1*1, or (1 + 0) * 0)
  return f > 0.0 ? (1.0 - (1.0 - f) * (1.0 - x)) + 0.0 : 0.0 + (1.0 + f) * x;
}
__device__ __forceinline__ void cp_adjust_body(const double* __restrict__ tqt,
                                               const double* __restrict__ a, double scale,
                                               double* __restrict__ out, int n, int ld) {
  const int row = blockIdx.y;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= n) return;
  const size_t at = (size_t)row * ld + col;
  out[at] = cp_adjust_value(tqt[at], a[at], scale);
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

// ---- ConstraintPropagation against a Q of K <= n directed entries (r_e, c_e, v_e) -----------
// T Q T = sum_e v_e T[:, r_e] T[c_e, :] = U V^T with the (n, Kp) panels
//   U[i, e] = v_e Tt[r_e, i]   (Tt = T^T; T itself when T is symmetric),   V[j, e] = T[c_e, j],
// row-major with the entry index contiguous, Kp = round_up(max(K, 1), 16), columns [K, Kp) zero.
// k_cp_pair_panels: both panels are "read a row, write a column": 32 entries x 32 columns go
// through an LDS tile as in k_transpose, so reads and writes are 256-byte row segments.
// blockIdx.x: column block of T; blockIdx.y: 2 * (entry block) + (0: U, 1: V).
__device__ __forceinline__ void cp_pair_panels_body(const CpPairItem& m) {
  __shared__ double tile[32][33];
  const bool second = (blockIdx.y & 1) != 0;
  const int e0 = (blockIdx.y >> 1) * 32, i0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const double* __restrict__ src = second ? m.tv : m.tu;
  const int32_t* __restrict__ index = second ? m.cols : m.rows;
  double* __restrict__ dst = second ? m.V : m.U;
#pragma unroll
  for (int r = ty; r < 32; r += 8) {
    const int e = e0 + r, i = i0 + tx;
    double v = 0.0;
    if (e < m.k && i < m.n) {
      v = src[(size_t)index[e] * m.ld + i];
      if (!second) v = m.vals[e] * v;
    }
    tile[r][tx] = v;
  }
  __syncthreads();
#pragma unroll
  for (int r = ty; r < 32; r += 8) {
    const int i = i0 + r, e = e0 + tx;
    if (i < m.n && e < m.kp) dst[(size_t)i * m.kp + e] = tile[tx][r];
  }
}
__global__ __launch_bounds__(256) void k_cp_pair_panels(const CpPairItem m) {
  cp_pair_panels_body(m);
}
// (whole workgroups leave: the barrier inside is reached by all threads or none)
__global__ __launch_bounds__(256) void k_cp_pair_panels_g(const GroupOf<CpPairItem> g) {
  const CpPairItem& m = g.s[blockIdx.z];
  if ((int)blockIdx.x * 32 >= m.n || (int)(blockIdx.y >> 1) * 32 >= m.kp) return;
  cp_pair_panels_body(m);
}

// k_cp_pairs_adjust: out = adjust(A, (1 - alpha)^2 U V^T) -- the product and k_cp_adjust in one
// kernel that reads A once and writes it once.  A workgroup (4 waves) owns a 64 x 64 tile of the
// output, a wave a 32 x 32 quarter = 2 x 2 v_mfma_f64_16x16x4_f64 accumulators.  Operand tiles
// are [64][16] doubles in LDS with the chunk swizzle of gemm_f64.hip (16-byte chunk kc of row r
// at chunk position kc ^ ((r >> 1) & 7): the ds_write_b128 of the staging and the ds_read_b128
// of the fragments are conflict-free).  The K order is fixed (entry order, 16 at a time), no
// atomics: the same input gives the same bits, in a group as alone.
// sym != 0 (A and the entry list symmetric): only tiles ti <= tj are computed; the tile goes
// through LDS, the mirror tile is written transposed from it and a diagonal tile takes its lower
// half from its upper half -- the result is exactly symmetric.  Otherwise each lane writes the
// elements it read.  out may alias a either way: a tile's A is read before any of it is written,
// and no other workgroup reads it.  Padding columns [n, ld) are left alone, as k_cp_adjust does.
constexpr int kPairTile = 64;
__device__ __forceinline__ int pair_chunk_off(int row, int kc) {
  return row * 16 + ((2 * kc) ^ (row & 14));
}
__device__ __forceinline__ void cp_pairs_adjust_body(const CpPairItem& m, double scale) {
  typedef double v4f64 __attribute__((ext_vector_type(4)));
  // operand tiles (2 x 64 x 16 doubles) in the K loop, the staged output tile (pitch 65) after it
  __shared__ __attribute__((aligned(16))) double smem[kPairTile * (kPairTile + 1)];
  double* Us = smem;
  double* Vs = smem + kPairTile * 16;
  const int ti = blockIdx.y, tj = blockIdx.x;
  const int n = m.n, ld = m.ld, kp = m.kp;
  const bool sym = m.sym != 0;
  const int row0 = ti * kPairTile, col0 = tj * kPairTile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, li = lane & 15, lg = lane >> 4;

  v4f64 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (v4f64){0.0, 0.0, 0.0, 0.0};

  // staging: chunk c = tid + 256 q is row c >> 3, k-chunk c & 7 (rows clamped at the ragged edge:
  // what they produce is never written)
  const double2* usrc[2];
  const double2* vsrc[2];
  int lds_at[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = tid + 256 * q, r = c >> 3, kc = c & 7;
    usrc[q] = reinterpret_cast<const double2*>(m.U + (size_t)min(row0 + r, n - 1) * kp + 2 * kc);
    vsrc[q] = reinterpret_cast<const double2*>(m.V + (size_t)min(col0 + r, n - 1) * kp + 2 * kc);
    lds_at[q] = pair_chunk_off(r, kc);
  }
  for (int kt = 0; kt < kp; kt += 16) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      *reinterpret_cast<double2*>(Us + lds_at[q]) = usrc[q][kt / 2];
      *reinterpret_cast<double2*>(Vs + lds_at[q]) = vsrc[q][kt / 2];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      // k-slot lg of the two MFMA steps carries k = 8p + 2lg and 8p + 2lg + 1
      const int koff = (2 * (4 * p + lg)) ^ (li & 14);
      double2 fa[2], fb[2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
        fa[a] = *reinterpret_cast<const double2*>(Us + (wr * 32 + a * 16 + li) * 16 + koff);
#pragma unroll
      for (int b = 0; b < 2; ++b)
        fb[b] = *reinterpret_cast<const double2*>(Vs + (wc * 32 + b * 16 + li) * 16 + koff);
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a].x, fb[b].x, acc[a][b], 0, 0, 0);
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a].y, fb[b].y, acc[a][b], 0, 0, 0);
    }
    __syncthreads();  // (the fragments are read: the tiles may be overwritten, or become `stage`)
  }

  // D layout of v_mfma_f64_16x16x4_f64: lane l, reg r holds D[(l >> 4) + 4 r][l & 15]
  constexpr int kPitch = kPairTile + 1;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = wr * 32 + a * 16 + lg + 4 * r, lc = wc * 32 + b * 16 + li;
        const int row = row0 + lr, col = col0 + lc;
        if (row >= n || col >= n) continue;
        const size_t at = (size_t)row * ld + col;
        const double v = cp_adjust_value(acc[a][b][r], m.a[at], scale);
        if (sym) smem[lr * kPitch + lc] = v;
        else m.out[at] = v;
      }
  if (!sym) return;  // (uniform)
  __syncthreads();
  const bool diagonal = ti == tj;
  for (int at = tid; at < kPairTile * kPairTile; at += 256) {
    const int lr = at >> 6, lc = at & 63;
    if (row0 + lr < n && col0 + lc < n)
      m.out[(size_t)(row0 + lr) * ld + col0 + lc] =
          diagonal && lr > lc ? smem[lc * kPitch + lr] : smem[lr * kPitch + lc];
    // the mirror tile: its row lr is column lr of this one
    if (!diagonal && col0 + lr < n && row0 + lc < n)
      m.out[(size_t)(col0 + lr) * ld + row0 + lc] = smem[lc * kPitch + lr];
  }
}
__global__ __launch_bounds__(256) void k_cp_pairs_adjust(const CpPairItem m, double scale) {
  if (m.sym != 0 && blockIdx.x < blockIdx.y) return;
  cp_pairs_adjust_body(m, scale);
}
__global__ __launch_bounds__(256) void k_cp_pairs_adjust_g(const GroupOf<CpPairItem> g,
                                                           double scale) {
  const CpPairItem& m = g.s[blockIdx.z];
  if ((int)blockIdx.x * kPairTile >= m.n || (int)blockIdx.y * kPairTile >= m.n) return;
  if (m.sym != 0 && blockIdx.x < blockIdx.y) return;
  cp_pairs_adjust_body(m, scale);
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
void launch_affinity_integration_pairs(hipStream_t s, const double* a, const int32_t* rows,
                                       const int32_t* cols, const double* vals, int k,
                                       double* orig, double* out, int n, int ld, int type) {
  const int eb = (k + 255) / 256;
  if (k > 0)
    hipLaunchKernelGGL(k_affinity_integration_pairs_gather, dim3(eb), dim3(256), 0, s, a, rows,
                       cols, k, ld, orig);
  hipLaunchKernelGGL(k_affinity_integration_pairs, dim3((n + 255) / 256, n), dim3(256), 0, s, a,
                     out, n, ld, type);
  if (k > 0)
    hipLaunchKernelGGL(k_affinity_integration_pairs_patch, dim3(eb), dim3(256), 0, s, orig, rows,
                       cols, vals, k, ld, type, out);
}
void launch_pairs_to_dense(hipStream_t s, const int32_t* rows, const int32_t* cols,
                           const double* vals, int k, int ld, double* q) {
  if (k > 0)
    hipLaunchKernelGGL(k_pairs_to_dense, dim3((k + 255) / 256), dim3(256), 0, s, rows, cols, vals,
                       k, ld, q);
}
int cp_pair_panel_width(int k) { return (std::max(k, 1) + 15) / 16 * 16; }
void launch_cp_pair_panels(hipStream_t s, const CpPairItem& m) {
  hipLaunchKernelGGL(k_cp_pair_panels, dim3((m.n + 31) / 32, 2 * ((m.kp + 31) / 32)), dim3(256), 0,
                     s, m);
}
void launch_cp_pairs_adjust(hipStream_t s, const CpPairItem& m, double scale) {
  const int nt = (m.n + kPairTile - 1) / kPairTile;
  hipLaunchKernelGGL(k_cp_pairs_adjust, dim3(nt, nt), dim3(256), 0, s, m, scale);
}
static GroupOf<CpPairItem> cp_pair_pack(const CpPairItem* items, int count, int* nmax,
                                        int* kpmax) {
  GroupOf<CpPairItem> g;
  memset(&g, 0, sizeof(g));
  *nmax = *kpmax = 0;
  for (int z = 0; z < count && z < kGroupMax; ++z) {
    if (items[z].n <= 0) continue;
    g.s[z] = items[z];
    *nmax = std::max(*nmax, items[z].n);
    *kpmax = std::max(*kpmax, items[z].kp);
  }
  return g;
}
void launch_cp_pair_panels_group(hipStream_t s, const CpPairItem* items, int count) {
  int nmax, kpmax;
  const GroupOf<CpPairItem> g = cp_pair_pack(items, count, &nmax, &kpmax);
  if (nmax == 0) return;
  hipLaunchKernelGGL(k_cp_pair_panels_g, dim3((nmax + 31) / 32, 2 * ((kpmax + 31) / 32), count),
                     dim3(256), 0, s, g);
}
void launch_cp_pairs_adjust_group(hipStream_t s, const CpPairItem* items, int count,
                                  double scale) {
  int nmax, kpmax;
  const GroupOf<CpPairItem> g = cp_pair_pack(items, count, &nmax, &kpmax);
  if (nmax == 0) return;
  const int nt = (nmax + kPairTile - 1) / kPairTile;
  hipLaunchKernelGGL(k_cp_pairs_adjust_g, dim3(nt, nt, count), dim3(256), 0, s, g, scale);
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
