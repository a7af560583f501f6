// sc_stage_tridiag / sc_stage_tridiag_values / sc_stage_td_backtransform: the three steps of the
// dense symmetric route (eig_dense.hip), each alone, through the launchers dense_spectrum and
// dense_vectors (eig_driver.hip) call (tests).  Every entry owns its device memory: buffers of the
// arena's shapes (row pitch matrix_ld(n), td_panel, td_work, the GEMM's split-K scratch) that
// start as quiet NaNs -- padding columns, workspaces and results alike -- so that anything read
// outside what the kernels were given, or a result nobody wrote, shows in what is copied out.
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
