// sc_stage_tridiag / sc_stage_tridiag_values / sc_stage_td_backtransform: the three steps of the
// dense symmetric route (eig_dense.hip), each alone, through the launchers dense_spectrum and
// dense_vectors (eig_driver.hip) call (tests).  Every entry owns its device memory: buffers of the
// arena's shapes (row pitch matrix_ld(n), td_panel, td_work, the GEMM's split-K scratch) that
// start as quiet NaNs -- padding columns, workspaces and results alike -- so that anything read
// outside what the kernels were given, or a result nobody wrote, shows in what is copied out.
// sc_stage_hessenberg / sc_stage_general_ritz / sc_stage_arnoldi_state (below them): the same for
// the general path -- hessenberg.hip, the Rayleigh-Ritz kernels of eig_general.hip, and the state
// a block Arnoldi solve of gen_topk leaves in the arena.
#include <limits>

#include "handle.h"

namespace {
// device buffers of one call, freed however the call returns
struct DenseStage {
  sc_handle h;
  hipStream_t s;
  std::vector<void*> owned;
  std::vector<double> fill;
  explicit DenseStage(sc_handle handle) : h(handle), s(handle->stream) {}
  ~DenseStage() {
    (void)hipStreamSynchronize(s);
    for (void* q : owned) (void)hipFree(q);
  }
  // `doubles` doubles of quiet NaNs; then, if src != nullptr, its first `count` doubles from src
  int buffer(size_t doubles, const double* src, size_t count, double** out) {
    void* d = nullptr;
    SC_HIP(h, hipMalloc(&d, std::max<size_t>(doubles, 1) * sizeof(double)));
    owned.push_back(d);
    fill.assign(doubles, std::numeric_limits<double>::quiet_NaN());
    if (src) std::copy(src, src + count, fill.begin());
    SC_HIP(h, hipMemcpyAsync(d, fill.data(), doubles * sizeof(double), hipMemcpyHostToDevice, s));
    SC_HIP(h, hipStreamSynchronize(s));  // (`fill` is reused)
    *out = reinterpret_cast<double*>(d);
    return SC_OK;
  }
  // an (n, n) matrix at the arena's pitch: NaN padding, then the rows of src
  int matrix(const double* src, int n, int ld, double** out) {
    SC_TRY(buffer((size_t)n * ld, nullptr, 0, out));
    return h2d_matrix(h, src, n, n, *out, ld);  // (same stream: after the fill)
  }
  int vector_out(const double* src, int n, double* dst) {
    if (!dst) return SC_OK;
    SC_HIP(h, hipMemcpyAsync(dst, src, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    return SC_OK;
  }
};

// the smallest n at which the arena's td_work (5 n + 2048 doubles) holds what
// launch_tridiagonalize_blocked lays out in it (2 n + 32 * 66 + (n + 6) / 8); the product takes
// the dense route above kDenseMax rows only
constexpr int kStageTridiagMin = 32;
}  // namespace

extern "C" int sc_stage_tridiag(sc_handle h, const double* m, int n, const double* c,
                                const double* p, double* d, double* e, double* tau,
                                double* reflectors) {
  if (!h) return SC_ERR_INVALID;
  if (!m || n <= 0) return fail(h, SC_ERR_INVALID, "sc_stage_tridiag: m must be (n, n)");
  if (n < kStageTridiagMin)
    return fail(h, SC_ERR_UNSUPPORTED, "sc_stage_tridiag: n >= 32 (the dense route runs above 128)");
  SC_HIP(h, hipSetDevice(h->device));
  DenseStage st(h);
  const int ld = matrix_ld(n);
  double *A, *dd, *de, *dtau, *panel, *work, *splitk;
  SC_TRY(st.matrix(m, n, ld, &A));
  if (c || p) {
    // Op = diag(p) + diag(c) m diag(c), as dense_spectrum forms it (a NULL one: c = 1 / p = 0)
    std::vector<double> dflt(n, c ? 0.0 : 1.0);
    double *dc, *dp, *M;
    SC_TRY(st.buffer(n, c ? c : dflt.data(), n, &dc));
    SC_TRY(st.buffer(n, p ? p : dflt.data(), n, &dp));
    SC_TRY(st.buffer((size_t)n * ld, nullptr, 0, &M));
    launch_td_materialize(st.s, A, ld, n, dc, dp, M);
    A = M;
  }
  SC_TRY(st.buffer(n, nullptr, 0, &dd));
  SC_TRY(st.buffer(n, nullptr, 0, &de));
  SC_TRY(st.buffer(n, nullptr, 0, &dtau));
  SC_TRY(st.buffer((size_t)n * 128, nullptr, 0, &panel));
  SC_TRY(st.buffer(5 * (size_t)n + 2048, nullptr, 0, &work));
  SC_TRY(st.buffer(gemm_splitk_workspace_bytes() / sizeof(double), nullptr, 0, &splitk));
  launch_tridiagonalize_blocked(st.s, A, ld, n, dd, de, dtau, panel, work, splitk);
  SC_TRY(check_last(h, "tridiagonalisation launch"));
  SC_TRY(st.vector_out(dd, n, d));
  SC_TRY(st.vector_out(de, n, e));
  SC_TRY(st.vector_out(dtau, n, tau));
  if (reflectors) return d2h_matrix(h, A, ld, n, n, reflectors);
  SC_HIP(h, hipStreamSynchronize(st.s));
  return SC_OK;
}

extern "C" int sc_stage_tridiag_values(sc_handle h, const double* d, const double* e, int n,
                                       double* values_desc) {
  if (!h) return SC_ERR_INVALID;
  if (!d || n <= 0 || (n > 1 && !e) || !values_desc)
    return fail(h, SC_ERR_INVALID, "sc_stage_tridiag_values: d (n), e (n - 1), values (n)");
  SC_HIP(h, hipSetDevice(h->device));
  DenseStage st(h);
  double *dd, *de, *theta, *work;
  SC_TRY(st.buffer(n, d, n, &dd));
  SC_TRY(st.buffer(n, e, n - 1, &de));  // (e[n - 1] stays NaN: nothing may read it)
  SC_TRY(st.buffer(n, nullptr, 0, &theta));
  SC_TRY(st.buffer((size_t)n + 4, nullptr, 0, &work));
  launch_tridiagonal_eigenvalues(st.s, dd, de, n, theta, work);
  SC_TRY(check_last(h, "tridiagonal eigenvalue launch"));
  SC_TRY(st.vector_out(theta, n, values_desc));
  SC_HIP(h, hipStreamSynchronize(st.s));
  return SC_OK;
}

extern "C" int sc_stage_td_backtransform(sc_handle h, const double* reflectors, const double* tau,
                                         int n, double* z, int cols, int flags) {
  if (!h) return SC_ERR_INVALID;
  if (!reflectors || !tau || !z || n <= 0 || cols <= 0 || (flags & ~SC_TD_BACKTRANSFORM_GLOBAL))
    return fail(h, SC_ERR_INVALID, "sc_stage_td_backtransform: reflectors (n, n), tau (n), z (n, cols)");
  SC_HIP(h, hipSetDevice(h->device));
  DenseStage st(h);
  const int ld = matrix_ld(n);
  const int lde = round_up(n, 16);
  double *A, *dtau, *E, *Eio;
  SC_TRY(st.matrix(reflectors, n, ld, &A));
  SC_TRY(st.buffer(n, tau, n, &dtau));
  // the columns as dense_vectors hands them over: column-major on the host, column q at q * lde
  // (the rows past n, zeros there, are NaNs here: the kernel owns rows < n only)
  std::vector<double> zc((size_t)lde * cols, std::numeric_limits<double>::quiet_NaN());
  for (int r = 0; r < n; ++r)
    for (int q = 0; q < cols; ++q) zc[(size_t)q * lde + r] = z[(size_t)r * cols + q];
  SC_TRY(st.buffer(zc.size(), zc.data(), zc.size(), &E));
  SC_TRY(st.buffer((size_t)n * cols, nullptr, 0, &Eio));
  launch_td_backtransform(st.s, A, ld, n, dtau, E, lde, cols,
                          (flags & SC_TD_BACKTRANSFORM_GLOBAL) != 0);
  // ... and as sc_stage_sym_eig / sc_get_eigenvectors read them back
  launch_colmajor_to_rowmajor(st.s, E, lde, n, cols, Eio, cols);
  SC_TRY(check_last(h, "back-transform launch"));
  return d2h_matrix(h, Eio, cols, n, cols, z);
}

// ------------------------------------------------------------------------------
// The general (non-symmetric) path, DESIGN 3.8: the Hessenberg reduction alone, the Rayleigh-Ritz
// kernels on given data, and what a block Arnoldi solve left behind.
// ------------------------------------------------------------------------------
extern "C" int sc_stage_hessenberg(sc_handle h, const double* m, int n, double* packed,
                                   double* tau, double* scale) {
  if (!h) return SC_ERR_INVALID;
  if (!m || n <= 0) return fail(h, SC_ERR_INVALID, "sc_stage_hessenberg: m must be (n, n), n >= 1");
  SC_HIP(h, hipSetDevice(h->device));
  DenseStage st(h);
  const int ld = matrix_ld(n);
  double *B, *absmax, *dtau, *vwork;
  SC_TRY(st.matrix(m, n, ld, &B));
  SC_TRY(st.buffer(4, nullptr, 0, &absmax));
  SC_TRY(st.buffer(n, nullptr, 0, &dtau));
  SC_TRY(st.buffer(5 * (size_t)n + 2048, nullptr, 0, &vwork));  // (the arena's td_work)
  double eig_scale = 1.0;
  SC_TRY(hessenberg_reduce_scaled(h, B, ld, n, absmax, dtau, vwork, &eig_scale));
  if (scale) *scale = eig_scale;
  SC_TRY(st.vector_out(dtau, n, tau));
  if (packed) return d2h_matrix(h, B, ld, n, n, packed);
  SC_HIP(h, hipStreamSynchronize(st.s));
  return SC_OK;
}

namespace {
// columns [0, cols) of a column-major device array (column c at src + c * ldv) -> (n, cols)
// row-major on the host
int columns_out(sc_handle h, const double* src, int ldv, int n, int cols, double* dst) {
  if (!dst) return SC_OK;
  std::vector<double> t((size_t)cols * n);
  SC_TRY(d2h_matrix(h, src, ldv, cols, n, t.data()));
  for (int c = 0; c < cols; ++c)
    for (int r = 0; r < n; ++r) dst[(size_t)r * cols + c] = t[(size_t)c * n + r];
  return SC_OK;
}
}  // namespace

extern "C" int sc_stage_general_ritz(sc_handle h, const double* q, const double* opq, int n, int m,
                                     const double* yre, const double* yim, const double* theta_re,
                                     const double* theta_im, int cols, double* vre, double* vim,
                                     double* resid, double* pre, double* pim, double* e,
                                     const int32_t* codes, uint64_t seed, double* w) {
  if (!h) return SC_ERR_INVALID;
  if (!yre || !yim || n <= 0 || m <= 0 || m > kEigBasisCap || cols <= 0 || cols > m)
    return fail(h, SC_ERR_INVALID,
                "sc_stage_general_ritz: yre, yim (m, cols), 1 <= cols <= m <= 128, n >= 1");
  if (!q && (m != n || n > kGenMax))
    return fail(h, SC_ERR_INVALID, "sc_stage_general_ritz: q = NULL (identity) needs m = n <= 64");
  if (resid && (!q || !opq || !theta_re || !theta_im))
    return fail(h, SC_ERR_INVALID, "sc_stage_general_ritz: resid needs q, opq, theta_re, theta_im");
  if ((codes != nullptr) != (w != nullptr))
    return fail(h, SC_ERR_INVALID, "sc_stage_general_ritz: codes (8) and w (n, 8) go together");
  if (codes)
    for (int j = 0; j < kEigBlock; ++j)
      if (codes[j] < -1 || codes[j] >= 2 * cols)
        return fail(h, SC_ERR_INVALID, "sc_stage_general_ritz: codes are -1 or 2 * column + part");
  SC_HIP(h, hipSetDevice(h->device));
  DenseStage st(h);
  hipStream_t s = st.s;
  const int ldv = round_up(n, 16);
  double *Q = nullptr, *OpQ = nullptr, *Yre, *Yim, *Vre, *Vim, *E;
  if (q) {
    SC_TRY(st.buffer((size_t)n * kLdq, nullptr, 0, &Q));
    SC_TRY(h2d_matrix(h, q, n, m, Q, kLdq));
  }
  if (opq) {
    SC_TRY(st.buffer((size_t)n * kLdq, nullptr, 0, &OpQ));
    SC_TRY(h2d_matrix(h, opq, n, m, OpQ, kLdq));
  }
  SC_TRY(st.buffer((size_t)kLdq * kLdq, nullptr, 0, &Yre));
  SC_TRY(h2d_matrix(h, yre, m, cols, Yre, kLdq));
  SC_TRY(st.buffer((size_t)kLdq * kLdq, nullptr, 0, &Yim));
  SC_TRY(h2d_matrix(h, yim, m, cols, Yim, kLdq));
  SC_TRY(st.buffer((size_t)ldv * cols, nullptr, 0, &Vre));
  SC_TRY(st.buffer((size_t)ldv * cols, nullptr, 0, &Vim));
  SC_TRY(st.buffer((size_t)ldv * cols, nullptr, 0, &E));
  SC_HIP(h, hipStreamSynchronize(s));  // (the inputs are the caller's pageable memory)
  if (resid) {
    double *tre, *tim, *partial, *dres;
    SC_TRY(st.buffer(kLdq, theta_re, cols, &tre));
    SC_TRY(st.buffer(kLdq, theta_im, cols, &tim));
    SC_TRY(st.buffer((size_t)gen_residual_blocks(n) * 32, nullptr, 0, &partial));
    SC_TRY(st.buffer(kLdq, nullptr, 0, &dres));
    gen_residuals(s, Q, OpQ, m, n, Yre, Yim, tre, tim, cols, partial, dres);
    SC_TRY(check_last(h, "residual launch"));
    SC_TRY(st.vector_out(dres, cols, resid));
  }
  launch_gen_ritz(s, Q, q ? kLdq : 0, m, n, Yre, Yim, kLdq, cols, Vre, Vim, ldv);
  SC_TRY(check_last(h, "ritz vector launch"));
  SC_TRY(columns_out(h, Vre, ldv, n, cols, vre));
  SC_TRY(columns_out(h, Vim, ldv, n, cols, vim));
  launch_gen_phase(s, Vre, Vim, ldv, n, cols, E, ldv);
  SC_TRY(check_last(h, "eigenvector normalisation launch"));
  SC_TRY(columns_out(h, Vre, ldv, n, cols, pre));
  SC_TRY(columns_out(h, Vim, ldv, n, cols, pim));
  SC_TRY(columns_out(h, E, ldv, n, cols, e));
  if (codes) {
    void* dcodes = nullptr;
    SC_HIP(h, hipMalloc(&dcodes, kEigBlock * sizeof(int)));
    st.owned.push_back(dcodes);
    SC_HIP(h, hipMemcpyAsync(dcodes, codes, kEigBlock * sizeof(int), hipMemcpyHostToDevice, s));
    double* W;
    SC_TRY(st.buffer((size_t)n * kEigBlock, nullptr, 0, &W));
    launch_gen_gather(s, Vre, Vim, ldv, n, reinterpret_cast<const int*>(dcodes), seed, W);
    SC_TRY(check_last(h, "restart block launch"));
    SC_TRY(st.vector_out(W, n * kEigBlock, w));
  }
  SC_HIP(h, hipStreamSynchronize(s));
  return SC_OK;
}

// What the last block Arnoldi solve of gen_topk on this handle left on the device, copied out;
// read-only like sc_stage_krylov_state (eig_driver.hip).  Q[:, 0:m], Q2[:, 0:m] = Op Q and
// T[0:m, 0:m] = H are what the solve's final check read: the exit path (k_gen_ritz, k_gen_phase)
// writes Vre / Vim / E only, and whatever brings a new problem, regrows the arena or starts
// another solve resets arnoldi_m.
extern "C" int sc_stage_arnoldi_state(sc_handle h, int32_t* info, double* q, double* opq,
                                      double* hm, double* cl, double* cr, double* p) {
  if (!h) return SC_ERR_INVALID;
  if (!info) return fail(h, SC_ERR_INVALID, "arnoldi state: info is NULL");
  if (h->arnoldi_m <= 0)
    return fail(h, SC_ERR_INVALID,
                "arnoldi state: the last solve on this handle was not block Arnoldi (a symmetric "
                "solve or a dense general route), or none has run");
  SC_HIP(h, hipSetDevice(h->device));
  const int m = h->arnoldi_m, n = h->arnoldi_n;
  memset(info, 0, 8 * sizeof(int32_t));
  info[0] = m;
  info[1] = n;
  info[2] = h->arnoldi_wide ? 1 : 0;
  info[3] = h->arnoldi_cycles;
  info[4] = h->arnoldi_passes;
  info[5] = h->arnoldi_negate ? 1 : 0;
  hipStream_t s = h->stream;
  const size_t row = (size_t)m * sizeof(double), pitch = (size_t)kLdq * sizeof(double);
  const size_t vec = (size_t)n * sizeof(double);
  if (q) SC_HIP(h, hipMemcpy2DAsync(q, row, h->Q.p, pitch, row, n, hipMemcpyDeviceToHost, s));
  if (opq) SC_HIP(h, hipMemcpy2DAsync(opq, row, h->Q2.p, pitch, row, n, hipMemcpyDeviceToHost, s));
  if (hm) SC_HIP(h, hipMemcpy2DAsync(hm, row, h->T.p, pitch, row, m, hipMemcpyDeviceToHost, s));
  // (a solve with the sign turned read -cl and -p from gneg: launch_negate2's layout)
  const double* dcl = ptr<double>(h->cvec);
  const double* dp = ptr<double>(h->pvec);
  if (h->arnoldi_negate) {
    dcl = ptr<double>(h->gneg);
    dp = ptr<double>(h->gneg) + round_up(n, 16);
  }
  if (cl) SC_HIP(h, hipMemcpyAsync(cl, dcl, vec, hipMemcpyDeviceToHost, s));
  if (cr) SC_HIP(h, hipMemcpyAsync(cr, h->crvec.p, vec, hipMemcpyDeviceToHost, s));
  if (p) SC_HIP(h, hipMemcpyAsync(p, dp, vec, hipMemcpyDeviceToHost, s));
  SC_HIP(h, hipStreamSynchronize(s));
  return SC_OK;
}
