// Host side of the constraint operators (reference constraint.py:95-164): the resident
// constraint (a dense matrix, the band of ConstraintMatrix, constraint.py:167-207, or a list of
// directed entries) and the GEMM chain of ConstraintPropagation; kernels in constraint.hip and
// gemm_f64.hip.
#include <algorithm>
#include <cmath>
#include <limits>
#include <utility>
#include <vector>

#include "handle.h"

// ------------------------------------------------------------------------------
// N3: constraints (reference constraint.py:95-164)
// ------------------------------------------------------------------------------
// exact symmetry of a resident (n, ld) matrix; one 4-byte D2H + stream sync
int device_is_symmetric(sc_handle h, const double* m, int n, int ld, bool* out) {
  SC_TRY(grow(h, h->symflag, 16));
  const int one = 1;
  int result = 0;
  SC_HIP(h, hipMemcpyAsync(h->symflag.p, &one, sizeof(int), hipMemcpyHostToDevice, h->stream));
  launch_symmetry_flag(h->stream, m, n, ld, ptr<int>(h->symflag));
  SC_HIP(h, hipMemcpyAsync(&result, h->symflag.p, sizeof(int), hipMemcpyDeviceToHost,
                           h->stream));
  SC_HIP(h, hipStreamSynchronize(h->stream));
  *out = result != 0;
  return SC_OK;
}

// ConstraintPropagation.adjust_affinity (constraint.py:138-164):  out may alias a.
//   P = alpha D^-1/2 A D^-1/2,  T = (I - P)^-1 = prod_{j>=0} (I + P^(2^j))  (rho(P) <= |alpha|),
//   F = (1 - alpha)^2 T Q T,  out = F > 0 ? 1 - (1 - F)(1 - A) : (1 + F) A.
// Every product runs on the fp64 MFMA GEMM (C = X Y^T).  For a symmetric A all factors
// are symmetric and commute, so squarings and T updates compute the upper tile triangle
// only; a general A carries explicit transposes instead.
// `banded`: Q is the matrix sc_set_constraint_band describes by `band` (n - 1 values, none for
// n = 1); q is not read and T^T Q^T is one streaming pass instead of a GEMM.
// factors (I + P^(2^j)), j = 0 .. steps-1, of the Neumann product for this alpha (they leave a
// remainder of P^(2^steps)); the refusals of the device route
static int neumann_steps(sc_handle h, double alpha, int* out) {
  const double mag = fabs(alpha);
  if (!(mag < 1.0))
    return fail(h, SC_ERR_UNSUPPORTED,
                "ConstraintPropagation on the device needs |constraint_propagation_alpha| < 1");
  int steps = 0;
  if (mag > 0.0) {
    double rem = mag;
    while (rem > 1e-18 && steps < 18) {
      rem *= rem;
      ++steps;
    }
    if (rem > 1e-18)
      return fail(h, SC_ERR_UNSUPPORTED,
                  "constraint_propagation_alpha too close to 1 for the Neumann product");
  }
  *out = steps;
  return SC_OK;
}

// A resident entry list on the device (sc_set_constraint_pairs): Q[rows[e], cols[e]] = vals[e]
struct DevPairs {
  const int32_t* rows = nullptr;
  const int32_t* cols = nullptr;
  const double* vals = nullptr;
  int k = 0;
};
static DevPairs resident_pairs(sc_handle h) {
  DevPairs p;
  p.k = h->pairs_count;
  p.vals = ptr<double>(h->Cpairs);
  p.rows = reinterpret_cast<const int32_t*>(p.vals + p.k);
  p.cols = p.rows + p.k;
  return p;
}

// `pairs` (k <= n entries, or nullptr): Q is that list; neither q nor band is read, and the last
// stage -- T^T Q^T, T X^T and the adjustment -- is the panels U, V and one kernel that forms
// U V^T tile by tile and adjusts A with it (constraint.hip).  The panels take two work matrices
// the chain has left idle; a symmetric A then needs four cp[] matrices instead of five.
static int constraint_propagation(sc_handle h, const double* a, bool sym_a, const double* q,
                                  bool sym_q, const double* band, bool banded,
                                  const DevPairs* pairs, double alpha, double* out, int n,
                                  int ld) {
  hipStream_t s = h->stream;
  int steps = 0;
  SC_TRY(neumann_steps(h, alpha, &steps));
  if (pairs && pairs->k == 0) {  // Q = 0: F = 0 and the adjustment is the identity
    if (out != a)
      SC_HIP(h, hipMemcpy2DAsync(out, (size_t)ld * sizeof(double), a, (size_t)ld * sizeof(double),
                                 (size_t)n * sizeof(double), n, hipMemcpyDeviceToDevice, s));
    return SC_OK;
  }
  const size_t bytes = (size_t)n * ld * sizeof(double);
  for (int i = 0; i < (pairs && sym_a ? 4 : 5); ++i) SC_TRY(grow(h, h->cp[i], bytes));
  SC_TRY(ensure_tilemap(h, n));
  double* P = ptr<double>(h->cp[0]);
  double* T = ptr<double>(h->cp[1]);
  double* Pn = ptr<double>(h->cp[2]);
  double* Tn = ptr<double>(h->cp[3]);
  double* X = ptr<double>(h->cp[4]);  // transposes (general A), then T Q^T
  double* ws = ptr<double>(h->splitk);
  const int2* tm = h->tilemap_cur;
  launch_row_stats(s, a, n, ld, ptr<double>(h->cut), ptr<double>(h->deg));  // deg = rowsum
  launch_cp_prepare(s, a, ptr<double>(h->deg), alpha, P, T, n, ld);          // T = I + P
  for (int j = 1; j < steps; ++j) {
    // Pn = P P
    if (sym_a) {
      launch_gemm_nt(s, P, ld, P, ld, Pn, ld, n, n, n, kEpiNone, true, ws, tm);
    } else {
      launch_transpose(s, P, X, n, ld);
      launch_gemm_nt(s, P, ld, X, ld, Pn, ld, n, n, n, kEpiNone, false, ws, nullptr);
    }
    std::swap(P, Pn);
    // Tn = T + T P
    if (sym_a) {
      launch_gemm_nt(s, T, ld, P, ld, Tn, ld, n, n, n, kEpiAdd, true, ws, tm, nullptr, T);
    } else {
      launch_transpose(s, P, X, n, ld);
      launch_gemm_nt(s, T, ld, X, ld, Tn, ld, n, n, n, kEpiAdd, false, ws, nullptr, nullptr, T);
    }
    std::swap(T, Tn);
  }
  // G^T = T^T Q^T  (X),  T Q T = T (G^T)^T  (Pn)
  const double* Tt = T;
  if (!sym_a) {
    launch_transpose(s, T, Tn, n, ld);
    Tt = Tn;
  }
  if (pairs) {
    // idle now: Pn, and Tn (symmetric A) or X (general A, whose Tn holds T^T)
    CpPairItem m;
    m.tu = Tt;
    m.tv = T;
    m.rows = pairs->rows;
    m.cols = pairs->cols;
    m.vals = pairs->vals;
    m.U = Pn;
    m.V = sym_a ? Tn : X;
    m.a = a;
    m.out = out;
    m.n = n;
    m.ld = ld;
    m.k = pairs->k;
    m.kp = cp_pair_panel_width(pairs->k);
    m.sym = sym_a && sym_q;
    launch_cp_pair_panels(s, m);
    launch_cp_pairs_adjust(s, m, (1.0 - alpha) * (1.0 - alpha));
    return check_last(h, "constraint propagation launch");
  }
  if (banded)
    launch_cp_band_product(s, Tt, band, X, n, ld);
  else
    launch_gemm_nt(s, Tt, ld, q, ld, X, ld, n, n, n, kEpiNone, false, ws, nullptr);
  const bool sym_f = sym_a && sym_q;
  launch_gemm_nt(s, T, ld, X, ld, Pn, ld, n, n, n, kEpiNone, sym_f, ws, sym_f ? tm : nullptr);
  launch_cp_adjust(s, Pn, a, (1.0 - alpha) * (1.0 - alpha), out, n, ld);
  return check_last(h, "constraint propagation launch");
}

// The same for up to kGroupMax symmetric affinities with banded constraints as ONE chain of
// grouped launches on stream s (a batch group's members, batch_group.hip): row sums, prepare,
// steps - 1 x (P <- P P, T <- T + T P), band product, T X^T, adjust -- 2 steps + 3 launches for
// the whole group where the members one by one take 13 each (and split their few tiles over K).
// `steps` depends on alpha alone.  Per member the elementwise arithmetic is the single route's;
// the products sum every tile's K whole.  The adjusted affinity replaces mem[z].A.  No
// allocation, no synchronisation.  A member's constraint may instead be an entry list (two
// launches for the pair members) or a dense symmetric matrix (mem[z].q: T Q^T by the full-output
// grouped product, T X^T, adjust).
int constraint_propagation_group(sc_handle lead, hipStream_t s, const CpGroupMember* mem,
                                 int count, double alpha) {
  int steps = 0;
  SC_TRY(neumann_steps(lead, alpha, &steps));
  if (count < 1 || count > kGroupMax)
    return fail(lead, SC_ERR_INVALID, "a constraint group holds 1 .. 16 members");
  FrontItem rs[kGroupMax];
  CpItem it[kGroupMax];
  GemmPairItem gm[kGroupMax];
  double *P[kGroupMax], *T[kGroupMax], *Pn[kGroupMax], *Tn[kGroupMax];
  memset(rs, 0, sizeof(rs));
  memset(it, 0, sizeof(it));
  bool any = false;
  for (int z = 0; z < count; ++z) {
    const CpGroupMember& m = mem[z];
    if (m.n <= 0) continue;
    any = true;
    P[z] = m.P;
    T[z] = m.T;
    Pn[z] = m.Pn;
    Tn[z] = m.Tn;
    rs[z].B2 = m.A;  // (launch_row_stats_group reads B2)
    rs[z].n = m.n;
    rs[z].ldn = m.ld;
    rs[z].rowmax = m.rowmax;
    rs[z].rowsum = m.deg;
    it[z] = CpItem{m.A, m.deg, m.P, m.T, m.n, m.ld};
  }
  if (!any) return SC_OK;
  auto product = [&](int z, const double* X, const double* Y, double* C, const double* add) {
    gm[z] = GemmPairItem();
    if (mem[z].n <= 0) return;
    gm[z].A = X;
    gm[z].B = Y;
    gm[z].lda = gm[z].ldb = gm[z].ldc = mem[z].ld;
    gm[z].C = C;
    gm[z].n = mem[z].n;
    gm[z].tilemap = mem[z].tilemap;
    gm[z].addend = add;
  };
  launch_row_stats_group(s, rs, count);           // deg = rowsum
  launch_cp_prepare_group(s, it, count, alpha);   // T = I + P
  for (int j = 1; j < steps; ++j) {
    for (int z = 0; z < count; ++z) product(z, P[z], nullptr, Pn[z], nullptr);  // Pn = P P
    launch_gemm_nt_pair_group(s, gm, count, kEpiNone);
    for (int z = 0; z < count; ++z) std::swap(P[z], Pn[z]);
    for (int z = 0; z < count; ++z) product(z, T[z], P[z], Tn[z], T[z]);        // Tn = T + T P
    launch_gemm_nt_pair_group(s, gm, count, kEpiAdd);
    for (int z = 0; z < count; ++z) std::swap(T[z], Tn[z]);
  }
  // The last stage, three times: the band members with the others idle, then the dense members,
  // then the pair members (a launch without live members is skipped).
  // X = T Q^T into the idle partner of T,  T Q T = T X^T into the idle partner of P
  bool any_band = false, any_pairs = false, any_dense = false;
  for (int z = 0; z < count; ++z) {
    it[z].n = 0;
    if (mem[z].n <= 0) continue;
    if (mem[z].q) {
      any_dense = true;
      continue;
    }
    if (mem[z].pairs) {
      any_pairs = any_pairs || mem[z].pk > 0;  // (no entries: Q = 0, A stays as it is)
      continue;
    }
    any_band = true;
    it[z] = CpItem{T[z], mem[z].band, Tn[z], nullptr, mem[z].n, mem[z].ld};
  }
  if (any_band) {
    launch_cp_band_product_group(s, it, count);
    for (int z = 0; z < count; ++z) {
      product(z, T[z], Tn[z], Pn[z], nullptr);
      if (mem[z].pairs || mem[z].q) gm[z] = GemmPairItem();
    }
    launch_gemm_nt_pair_group(s, gm, count, kEpiNone);
    for (int z = 0; z < count; ++z)
      if (it[z].n > 0) it[z] = CpItem{Pn[z], mem[z].A, mem[z].A, nullptr, mem[z].n, mem[z].ld};
    launch_cp_adjust_group(s, it, count, (1.0 - alpha) * (1.0 - alpha));
  }
  if (any_dense) {
    // X = T Q^T is not symmetric: every tile from its own operands (the full-output product);
    // T X^T = T Q T is, for a symmetric Q
    for (int z = 0; z < count; ++z) {
      product(z, T[z], mem[z].q, Tn[z], nullptr);
      if (!mem[z].q) gm[z] = GemmPairItem();
    }
    launch_gemm_nt_pair_group(s, gm, count, kEpiNone, true);
    for (int z = 0; z < count; ++z) {
      product(z, T[z], Tn[z], Pn[z], nullptr);
      if (!mem[z].q) gm[z] = GemmPairItem();
    }
    launch_gemm_nt_pair_group(s, gm, count, kEpiNone);
    for (int z = 0; z < count; ++z) {
      it[z].n = 0;
      if (mem[z].n > 0 && mem[z].q)
        it[z] = CpItem{Pn[z], mem[z].A, mem[z].A, nullptr, mem[z].n, mem[z].ld};
    }
    launch_cp_adjust_group(s, it, count, (1.0 - alpha) * (1.0 - alpha));
  }
  if (any_pairs) {
    // the panels into the idle partners of P and T (T is symmetric: it is its own transpose)
    CpPairItem pm[kGroupMax];
    memset(pm, 0, sizeof(pm));
    for (int z = 0; z < count; ++z) {
      const CpGroupMember& m = mem[z];
      if (m.n <= 0 || !m.pairs || m.pk <= 0) continue;
      if (m.pk > m.n)
        return fail(lead, SC_ERR_INVALID, "a grouped entry list holds at most n entries");
      CpPairItem& p = pm[z];
      p.tu = p.tv = T[z];
      p.rows = m.prows;
      p.cols = m.pcols;
      p.vals = m.pvals;
      p.U = Pn[z];
      p.V = Tn[z];
      p.a = p.out = m.A;
      p.n = m.n;
      p.ld = m.ld;
      p.k = m.pk;
      p.kp = cp_pair_panel_width(m.pk);
      p.sym = m.psym ? 1 : 0;
    }
    launch_cp_pair_panels_group(s, pm, count);
    launch_cp_pairs_adjust_group(s, pm, count, (1.0 - alpha) * (1.0 - alpha));
  }
  return check_last(lead, "grouped constraint propagation launch");
}

// cfg's constraint operator on `a` with the resident constraint (dense, banded or an entry
// list); out may alias a.
// The route of an entry list of K directed entries (derived, not tuned): AffinityIntegration
// always takes the list.  ConstraintPropagation takes it while K <= n: the pair stage then does
// at most n^3 of the dense stage's 3 n^3 flops and needs no n x n temporary beyond T.  For K > n
// the entries are scattered into the zero-filled Cq on the device and the dense stage runs.
int adjust_affinity(sc_handle h, const sc_config* cfg, const double* a, bool sym_a,
                           double* out, int n, int ld) {
  if (cfg->constraint_name == SC_CONSTRAINT_AFFINITY_INTEGRATION) {
    if (cfg->integration_type != SC_INTEGRATION_MAX &&
        cfg->integration_type != SC_INTEGRATION_AVERAGE)
      return fail(h, SC_ERR_INVALID, "Unsupported integration type");
    if (h->constraint_pairs) {
      const DevPairs p = resident_pairs(h);
      SC_TRY(grow(h, h->Cporig, (size_t)std::max(p.k, 1) * sizeof(double)));
      launch_affinity_integration_pairs(h->stream, a, p.rows, p.cols, p.vals, p.k,
                                        ptr<double>(h->Cporig), out, n, ld,
                                        cfg->integration_type);
    } else if (h->constraint_banded)
      launch_affinity_integration_band(h->stream, a, ptr<double>(h->Cband), out, n, ld,
                                       cfg->integration_type);
    else
      launch_affinity_integration(h->stream, a, ptr<double>(h->Cq), out, n, ld,
                                  cfg->integration_type);
    return check_last(h, "affinity integration launch");
  }
  if (cfg->constraint_name == SC_CONSTRAINT_PROPAGATION) {
    if (h->constraint_pairs) {
      const DevPairs p = resident_pairs(h);
      if (p.k <= n)
        return constraint_propagation(h, a, sym_a, nullptr, h->constraint_symmetric, nullptr,
                                      false, &p, cfg->constraint_alpha, out, n, ld);
      int steps = 0;
      SC_TRY(neumann_steps(h, cfg->constraint_alpha, &steps));  // (before Cq is allocated)
      const size_t bytes = (size_t)n * ld * sizeof(double);
      SC_TRY(grow(h, h->Cq, bytes));
      SC_HIP(h, hipMemsetAsync(h->Cq.p, 0, bytes, h->stream));
      launch_pairs_to_dense(h->stream, p.rows, p.cols, p.vals, p.k, ld, ptr<double>(h->Cq));
      return constraint_propagation(h, a, sym_a, ptr<double>(h->Cq), h->constraint_symmetric,
                                    nullptr, false, nullptr, cfg->constraint_alpha, out, n, ld);
    }
    return constraint_propagation(h, a, sym_a, ptr<double>(h->Cq), h->constraint_symmetric,
                                  ptr<double>(h->Cband), h->constraint_banded, nullptr,
                                  cfg->constraint_alpha, out, n, ld);
  }
  return fail(h, SC_ERR_INVALID, "constraint_name must be a ConstraintName");
}

// An entry list as the caller gives it (host memory): every index inside [0, n), every value
// finite, no position twice -- and whether it is symmetric (every (r, c, v) with r != c has its
// twin (c, r, v)), all on the host, O(K log K)
int validate_constraint_pairs(sc_handle h, const int32_t* rows, const int32_t* cols,
                              const double* vals, int count, int n, bool* symmetric) {
  if (count < 0 || (count > 0 && (!rows || !cols || !vals)))
    return fail(h, SC_ERR_INVALID, "a constraint entry list holds rows, cols and vals");
  std::vector<std::pair<int64_t, double>> at((size_t)count);
  for (int e = 0; e < count; ++e) {
    if (rows[e] < 0 || rows[e] >= n || cols[e] < 0 || cols[e] >= n)
      return fail(h, SC_ERR_INVALID, "constraint entry index outside [0, n)");
    if (!std::isfinite(vals[e]))
      return fail(h, SC_ERR_INVALID, "constraint entry values must be finite");
    at[e] = {(int64_t)rows[e] * n + cols[e], vals[e]};
  }
  std::sort(at.begin(), at.end());
  for (int e = 1; e < count; ++e)
    if (at[e].first == at[e - 1].first)
      return fail(h, SC_ERR_INVALID, "a constraint entry position is listed twice");
  bool sym = true;
  for (int e = 0; e < count && sym; ++e) {
    const int64_t r = at[e].first / n, c = at[e].first % n;
    if (r == c) continue;
    const auto twin = std::lower_bound(at.begin(), at.end(),
                                       std::make_pair(c * n + r, -HUGE_VAL));
    sym = twin != at.end() && twin->first == c * n + r && twin->second == at[e].second;
  }
  *symmetric = sym;
  return SC_OK;
}
// vals | rows | cols as Cpairs holds them: 16 bytes per entry
std::vector<double> pack_constraint_pairs(const int32_t* rows, const int32_t* cols,
                                          const double* vals, int count) {
  std::vector<double> packed((size_t)2 * count);
  if (count > 0) {
    memcpy(packed.data(), vals, (size_t)count * sizeof(double));
    int32_t* index = reinterpret_cast<int32_t*>(packed.data() + count);
    memcpy(index, rows, (size_t)count * sizeof(int32_t));
    memcpy(index + count, cols, (size_t)count * sizeof(int32_t));
  }
  return packed;
}

extern "C" int sc_set_constraint(sc_handle h, const double* q, int n) {
  if (!h) return SC_ERR_INVALID;
  if (!q || n <= 0) return fail(h, SC_ERR_INVALID, "constraint matrix must be (n, n)");
  SC_HIP(h, hipSetDevice(h->device));
  const int ld = matrix_ld(n);
  SC_TRY(grow(h, h->Cq, (size_t)n * ld * sizeof(double)));
  SC_TRY(h2d_matrix(h, q, n, n, ptr<double>(h->Cq), ld));
  SC_TRY(device_is_symmetric(h, ptr<double>(h->Cq), n, ld, &h->constraint_symmetric));
  h->have_constraint = true;
  h->constraint_banded = h->constraint_pairs = false;
  h->qn = n;
  return SC_OK;
}

// sc_set_constraint for a described source: read where it is (a device source in place, a narrow
// host source crossing the link at its own width), widened exactly into Cq by the ingest kernel,
// whose own flag is the symmetry -- one pass.  (Host fp64 keeps sc_set_constraint's copy and the
// separate pass: ingest_affinity_into.)
extern "C" int sc_set_constraint_array(sc_handle h, const sc_array* q) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_affinity_array(h, q, "constraint matrix"));
  SC_HIP(h, hipSetDevice(h->device));
  const int n = (int)q->rows, ld = matrix_ld(n);
  SC_TRY(grow(h, h->Cq, (size_t)n * ld * sizeof(double)));
  SC_TRY(grow(h, h->symflag, 16));
  h->have_constraint = false;
  // (symflag[0] is the affinity ingest's word and [1] the embedding rows': this one is [2])
  int* flag = ptr<int>(h->symflag) + 2;
  bool packed = false;  // (not read: the wait below comes whether or not the source was packed)
  SC_TRY(ingest_affinity_into(h, *q, ptr<double>(h->Cq), ld, flag, h->stream, &packed));
  int symmetric = 0;
  SC_HIP(h, hipMemcpyAsync(&symmetric, flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  SC_HIP(h, hipStreamSynchronize(h->stream));  // (and the source may be reused)
  h->constraint_symmetric = symmetric != 0;
  h->have_constraint = true;
  h->constraint_banded = h->constraint_pairs = false;
  h->qn = n;
  return SC_OK;
}

// ConstraintMatrix.compute_diagonals (constraint.py:188-201) without the matrix: n - 1 doubles
// up, nothing else (a band is symmetric by construction)
extern "C" int sc_set_constraint_band(sc_handle h, const double* band, int n) {
  if (!h) return SC_ERR_INVALID;
  if (n <= 0 || (!band && n > 1))
    return fail(h, SC_ERR_INVALID, "constraint band must hold n - 1 values");
  SC_HIP(h, hipSetDevice(h->device));
  const size_t bytes = (size_t)(n - 1) * sizeof(double);
  SC_TRY(grow(h, h->Cband, bytes));
  if (bytes > 0) {
    SC_HIP(h, hipMemcpyAsync(h->Cband.p, band, bytes, hipMemcpyHostToDevice, h->stream));
    // (pageable source: the caller's array may change once this returns)
    SC_HIP(h, hipStreamSynchronize(h->stream));
  }
  h->have_constraint = true;
  h->constraint_banded = true;
  h->constraint_pairs = false;
  h->constraint_symmetric = true;
  h->qn = n;
  return SC_OK;
}

// A constraint matrix given as its `count` non-zero entries: count x (4 + 4 + 8) bytes up,
// nothing else; symmetry is decided on the host while validating
extern "C" int sc_set_constraint_pairs(sc_handle h, const int32_t* rows, const int32_t* cols,
                                       const double* vals, int count, int n) {
  if (!h) return SC_ERR_INVALID;
  if (n <= 0) return fail(h, SC_ERR_INVALID, "constraint matrix must be (n, n)");
  bool symmetric = true;
  SC_TRY(validate_constraint_pairs(h, rows, cols, vals, count, n, &symmetric));
  SC_HIP(h, hipSetDevice(h->device));
  const size_t bytes = (size_t)count * 2 * sizeof(double);
  SC_TRY(grow(h, h->Cpairs, bytes));
  if (bytes > 0) {
    const std::vector<double> packed = pack_constraint_pairs(rows, cols, vals, count);
    SC_HIP(h, hipMemcpyAsync(h->Cpairs.p, packed.data(), bytes, hipMemcpyHostToDevice,
                             h->stream));
    SC_HIP(h, hipStreamSynchronize(h->stream));  // (pageable source)
  }
  h->have_constraint = true;
  h->constraint_banded = false;
  h->constraint_pairs = true;
  h->constraint_symmetric = symmetric;
  h->pairs_count = count;
  h->qn = n;
  return SC_OK;
}

extern "C" int sc_constraint_pairs_info(sc_handle h, int* count, size_t* pair_bytes) {
  if (!h) return SC_ERR_INVALID;
  if (count) *count = h->have_constraint && h->constraint_pairs ? h->pairs_count : 0;
  if (pair_bytes) *pair_bytes = h->Cpairs.bytes;
  return SC_OK;
}

extern "C" int sc_clear_constraint(sc_handle h) {
  if (!h) return SC_ERR_INVALID;
  h->have_constraint = false;
  h->constraint_banded = h->constraint_pairs = false;
  h->qn = 0;
  return SC_OK;
}

extern "C" int sc_constraint_info(sc_handle h, int* kind, int* n, size_t* band_bytes,
                                  size_t* dense_bytes) {
  if (!h) return SC_ERR_INVALID;
  if (kind)
    *kind = !h->have_constraint ? 0 : (h->constraint_pairs ? 3 : (h->constraint_banded ? 2 : 1));
  if (n) *n = h->have_constraint ? h->qn : 0;
  if (band_bytes) *band_bytes = h->Cband.bytes;
  if (dense_bytes) *dense_bytes = h->Cq.bytes;
  return SC_OK;
}

bool constraint_active(sc_handle h, const sc_config* cfg, bool before) {
  return cfg->constraint_name != SC_CONSTRAINT_NONE && h->have_constraint &&
         (cfg->constraint_before_refinement != 0) == before;
}

extern "C" int sc_apply_constraint(sc_handle h, const sc_config* cfg) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_config(h, cfg));
  if (!h->have_affinity) return fail(h, SC_ERR_INVALID, "no affinity resident");
  if (!h->have_constraint) return fail(h, SC_ERR_INVALID, "no constraint matrix resident");
  h->sweep_slot.clear();  // (a sweep on the unadjusted affinity)
  if (cfg->constraint_name == SC_CONSTRAINT_NONE)
    return fail(h, SC_ERR_INVALID, "no constraint operation configured");
  if (h->qn != h->n)
    return fail(h, SC_ERR_INVALID, "affinity and constraint matrix must have the same shape");
  if (h->constraint_applied)
    return fail(h, SC_ERR_INVALID, "the resident affinity is already constraint-adjusted");
  SC_HIP(h, hipSetDevice(h->device));
  SC_TRY(ensure_matrices(h, h->n, 0));
  SC_TRY(adjust_affinity(h, cfg, ptr<double>(h->A0), h->affinity_symmetric, ptr<double>(h->A0),
                         h->n, h->ldn));
  h->affinity_symmetric = h->affinity_symmetric && h->constraint_symmetric;
  h->have_cropval = false;
  h->constraint_applied = true;
  h->n_vec = 0;
  return SC_OK;
}

extern "C" int sc_stage_constraint(sc_handle h, const sc_config* cfg, const double* affinity,
                                   const double* q, int n, double* out) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_config(h, cfg));
  if (!affinity || !q || !out || n <= 0)
    return fail(h, SC_ERR_INVALID, "affinity and constraint matrix must be (n, n)");
  SC_TRY(sc_set_affinity(h, affinity, n));
  SC_TRY(sc_set_constraint(h, q, n));
  const int rc = sc_apply_constraint(h, cfg);
  sc_clear_constraint(h);
  SC_TRY(rc);
  return d2h_matrix(h, ptr<double>(h->A0), h->ldn, n, n, out);
}

// the same with the constraint matrix as a described source (sc_set_constraint_array)
extern "C" int sc_stage_constraint_array(sc_handle h, const sc_config* cfg, const double* affinity,
                                         const sc_array* q, int n, double* out) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_config(h, cfg));
  if (!affinity || !out || n <= 0)
    return fail(h, SC_ERR_INVALID, "affinity and constraint matrix must be (n, n)");
  SC_TRY(validate_affinity_array(h, q, "constraint matrix"));
  if (q->rows != n)
    return fail(h, SC_ERR_INVALID, "affinity and constraint matrix must have the same shape");
  SC_TRY(sc_set_affinity(h, affinity, n));
  SC_TRY(sc_set_constraint_array(h, q));
  const int rc = sc_apply_constraint(h, cfg);
  sc_clear_constraint(h);
  SC_TRY(rc);
  return d2h_matrix(h, ptr<double>(h->A0), h->ldn, n, n, out);
}

extern "C" int sc_stage_constraint_band(sc_handle h, const sc_config* cfg,
                                        const double* affinity, const double* band, int n,
                                        double* out) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_config(h, cfg));
  if (!affinity || !out || n <= 0 || (!band && n > 1))
    return fail(h, SC_ERR_INVALID, "affinity must be (n, n) and the band hold n - 1 values");
  SC_TRY(sc_set_affinity(h, affinity, n));
  SC_TRY(sc_set_constraint_band(h, band, n));
  const int rc = sc_apply_constraint(h, cfg);
  sc_clear_constraint(h);
  SC_TRY(rc);
  return d2h_matrix(h, ptr<double>(h->A0), h->ldn, n, n, out);
}

extern "C" int sc_stage_constraint_pairs(sc_handle h, const sc_config* cfg,
                                         const double* affinity, const int32_t* rows,
                                         const int32_t* cols, const double* vals, int count, int n,
                                         double* out) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_config(h, cfg));
  if (!affinity || !out || n <= 0)
    return fail(h, SC_ERR_INVALID, "affinity must be (n, n)");
  SC_TRY(sc_set_affinity(h, affinity, n));
  SC_TRY(sc_set_constraint_pairs(h, rows, cols, vals, count, n));
  const int rc = sc_apply_constraint(h, cfg);
  sc_clear_constraint(h);
  SC_TRY(rc);
  return d2h_matrix(h, ptr<double>(h->A0), h->ldn, n, n, out);
}

// ConstraintPropagation of `count` affinities with banded constraints as ONE grouped chain,
// through the launchers a constrained batch uses (tests).  Owns its device memory: per member the
// affinity and the four work matrices at the arena's row pitch, all of it -- padding columns and
// workspaces -- quiet NaNs before the inputs go in, so a read outside a matrix shows in the result.
// bands == nullptr: the members' constraints are entry lists (rows[z], cols[z], vals[z], counts[z]
// <= ns[z] entries) instead, in NaN-filled buffers of their own.  denses != nullptr: they are dense
// symmetric (ns[z], ns[z]) host matrices, each in a NaN-filled matrix of the arena's pitch
// (denses[z] == nullptr: idle member).
static int stage_constraint_group(sc_handle h, const sc_config* cfg, int count, const int32_t* ns,
                                  const double* const* affinities, const double* const* bands,
                                  const int32_t* const* rows, const int32_t* const* cols,
                                  const double* const* vals, const int32_t* counts,
                                  double* const* outs, const double* const* denses = nullptr) {
  SC_TRY(validate_config(h, cfg));
  if (count < 1 || count > kGroupMax || !ns || !affinities || !outs ||
      (!bands && !denses && (!rows || !cols || !vals || !counts)))
    return fail(h, SC_ERR_INVALID, "a constraint group holds 1 .. 16 members");
  auto is_idle = [&](int z) {
    return ns[z] == 0 || (bands && !bands[z] && ns[z] > 1) || (denses && !denses[z]);
  };
  bool list_symmetric[kGroupMax] = {};
  for (int z = 0; z < count; ++z) {
    if (ns[z] < 0) return fail(h, SC_ERR_INVALID, "n must not be negative (0: idle member)");
    // (larger tile grids get their order uploaded per size: one per handle at a time)
    if (gemm_tile_dim(ns[z]) > kTilemapTableMax)
      return fail(h, SC_ERR_UNSUPPORTED, "a member of the constraint group is larger than 8192");
    const bool idle = is_idle(z);
    if (!idle && (!affinities[z] || !outs[z]))
      return fail(h, SC_ERR_INVALID, "affinity must be (n, n) and the band hold n - 1 values");
    if (!idle && denses) {  // (the grouped chain's dense stage is the symmetric one)
      const int n = ns[z];
      for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
          if (!(denses[z][(size_t)i * n + j] == denses[z][(size_t)j * n + i]))
            return fail(h, SC_ERR_INVALID, "a grouped dense constraint must be symmetric");
    }
    if (!idle && !bands && !denses) {
      if (counts[z] > ns[z])
        return fail(h, SC_ERR_UNSUPPORTED,
                    "an entry list of more than n entries takes the dense route: not grouped");
      SC_TRY(validate_constraint_pairs(h, rows[z], cols[z], vals[z], counts[z], ns[z],
                                       &list_symmetric[z]));
    }
  }
  int steps = 0;
  SC_TRY(neumann_steps(h, cfg->constraint_alpha, &steps));  // (before anything is allocated)
  SC_HIP(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  struct Owned {  // freed however the function returns
    std::vector<void*> p;
    ~Owned() {
      for (void* q : p) (void)hipFree(q);
    }
  } owned;
  size_t largest = 16;
  for (int z = 0; z < count; ++z) largest = std::max(largest, (size_t)ns[z] * matrix_ld(ns[z]));
  // (one source for every fill, sized once: the copies out of it are in flight together)
  const std::vector<double> nans(largest, std::numeric_limits<double>::quiet_NaN());
  auto device_nan = [&](size_t doubles, double** out) -> int {
    void* d = nullptr;
    doubles = std::max<size_t>(doubles, 1);
    SC_HIP(h, hipMalloc(&d, doubles * sizeof(double)));
    owned.p.push_back(d);
    SC_HIP(h, hipMemcpyAsync(d, nans.data(), doubles * sizeof(double), hipMemcpyHostToDevice, s));
    *out = reinterpret_cast<double*>(d);
    return SC_OK;
  };
  CpGroupMember mem[kGroupMax];
  std::vector<double> packed[kGroupMax];  // (pageable sources of the entry uploads)
  for (int z = 0; z < count; ++z) {
    const int n = ns[z];
    if (is_idle(z)) continue;
    const int ld = matrix_ld(n);
    CpGroupMember& m = mem[z];
    double* band = nullptr;
    if (denses) {
      double* q_dev = nullptr;
      SC_TRY(device_nan((size_t)n * ld, &q_dev));
      SC_TRY(h2d_matrix(h, denses[z], n, n, q_dev, ld));  // (same stream: after the fill)
      m.q = q_dev;
    } else if (!bands) {
      double* packed_dev = nullptr;
      const int k = counts[z];
      SC_TRY(device_nan((size_t)2 * k, &packed_dev));
      if (k > 0) {
        packed[z] = pack_constraint_pairs(rows[z], cols[z], vals[z], k);
        SC_HIP(h, hipMemcpyAsync(packed_dev, packed[z].data(), (size_t)2 * k * sizeof(double),
                                 hipMemcpyHostToDevice, s));
      }
      m.pairs = true;
      m.psym = list_symmetric[z];
      m.pk = k;
      m.pvals = packed_dev;
      m.prows = reinterpret_cast<const int32_t*>(packed_dev + k);
      m.pcols = m.prows + k;
    }
    SC_TRY(device_nan((size_t)n * ld, &m.A));
    SC_TRY(device_nan((size_t)n * ld, &m.P));
    SC_TRY(device_nan((size_t)n * ld, &m.T));
    SC_TRY(device_nan((size_t)n * ld, &m.Pn));
    SC_TRY(device_nan((size_t)n * ld, &m.Tn));
    SC_TRY(device_nan(round_up(n, 16), &m.deg));
    SC_TRY(device_nan(round_up(n, 16), &m.rowmax));
    SC_TRY(device_nan(n - 1, &band));
    SC_TRY(h2d_matrix(h, affinities[z], n, n, m.A, ld));  // (same stream: after the fill)
    if (bands && n > 1)
      SC_HIP(h, hipMemcpyAsync(band, bands[z], (size_t)(n - 1) * sizeof(double),
                               hipMemcpyHostToDevice, s));
    SC_TRY(ensure_tilemap(h, n));
    m.band = band;
    m.tilemap = h->tilemap_cur;
    m.n = n;
    m.ld = ld;
  }
  SC_HIP(h, hipStreamSynchronize(s));  // (`nans` and the caller's bands are pageable)
  SC_TRY(constraint_propagation_group(h, s, mem, count, cfg->constraint_alpha));
  for (int z = 0; z < count; ++z)
    if (mem[z].n > 0) SC_TRY(d2h_matrix(h, mem[z].A, mem[z].ld, mem[z].n, mem[z].n, outs[z]));
  SC_HIP(h, hipStreamSynchronize(s));
  return SC_OK;
}

extern "C" int sc_stage_constraint_band_group(sc_handle h, const sc_config* cfg, int count,
                                              const int32_t* ns, const double* const* affinities,
                                              const double* const* bands, double* const* outs) {
  if (!h) return SC_ERR_INVALID;
  if (!bands) return fail(h, SC_ERR_INVALID, "a constraint group holds 1 .. 16 members");
  return stage_constraint_group(h, cfg, count, ns, affinities, bands, nullptr, nullptr, nullptr,
                                nullptr, outs);
}

// the same with each member's constraint as an entry list (sc_set_constraint_pairs)
extern "C" int sc_stage_constraint_pairs_group(sc_handle h, const sc_config* cfg, int count,
                                               const int32_t* ns,
                                               const double* const* affinities,
                                               const int32_t* const* rows,
                                               const int32_t* const* cols,
                                               const double* const* vals, const int32_t* counts,
                                               double* const* outs) {
  if (!h) return SC_ERR_INVALID;
  if (!rows || !cols || !vals || !counts)
    return fail(h, SC_ERR_INVALID, "a constraint group holds 1 .. 16 members");
  return stage_constraint_group(h, cfg, count, ns, affinities, nullptr, rows, cols, vals, counts,
                                outs);
}

// the same with each member's constraint as a dense symmetric (ns[z], ns[z]) host matrix
extern "C" int sc_stage_constraint_dense_group(sc_handle h, const sc_config* cfg, int count,
                                               const int32_t* ns,
                                               const double* const* affinities,
                                               const double* const* constraints,
                                               double* const* outs) {
  if (!h) return SC_ERR_INVALID;
  if (!constraints) return fail(h, SC_ERR_INVALID, "a constraint group holds 1 .. 16 members");
  return stage_constraint_group(h, cfg, count, ns, affinities, nullptr, nullptr, nullptr, nullptr,
                                nullptr, outs, constraints);
}

// ONE launch_gemm_nt_pair_group launch on host operands (tests): member z computes outs[z] =
// As[z] Bs[z]^T (+ addends[z]) for (ns[z], ns[z]) row-major matrices; Bs[z] == NULL: B = A.  The
// operands and the result live in matrices of the arena's row pitch whose every other element is a
// quiet NaN, and outs[z] receives all ns[z] x matrix_ld(ns[z]) elements of the result's buffer,
// padding columns included.  full = 0: the symmetric form (upper-triangle tiles and the mirror,
// for commuting symmetric operands); full != 0: every tile from its own operands.
extern "C" int sc_stage_gemm_pair_group(sc_handle h, int count, const int32_t* ns,
                                        const double* const* As, const double* const* Bs,
                                        const double* const* addends, double* const* outs,
                                        int epilogue, int full) {
  if (!h) return SC_ERR_INVALID;
  if (count < 1 || count > kGroupMax || !ns || !As || !outs)
    return fail(h, SC_ERR_INVALID, "a product group holds 1 .. 16 members");
  if (epilogue != kEpiNone && epilogue != kEpiAdd)
    return fail(h, SC_ERR_INVALID, "epilogue must be 0 (none) or the add epilogue");
  if (epilogue == kEpiAdd && !addends) return fail(h, SC_ERR_INVALID, "addends is NULL");
  for (int z = 0; z < count; ++z) {
    if (ns[z] < 0) return fail(h, SC_ERR_INVALID, "n must not be negative (0: idle member)");
    if (gemm_tile_dim(ns[z]) > kTilemapTableMax)
      return fail(h, SC_ERR_UNSUPPORTED, "a member of the product group is larger than 8192");
    if (ns[z] > 0 && (!As[z] || !outs[z] || (epilogue == kEpiAdd && !addends[z])))
      return fail(h, SC_ERR_INVALID, "NULL operand of a live member");
  }
  SC_HIP(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  struct Owned {  // freed however the function returns
    std::vector<void*> p;
    ~Owned() {
      for (void* q : p) (void)hipFree(q);
    }
  } owned;
  size_t largest = 16;
  for (int z = 0; z < count; ++z) largest = std::max(largest, (size_t)ns[z] * matrix_ld(ns[z]));
  const std::vector<double> nans(largest, std::numeric_limits<double>::quiet_NaN());
  auto device_matrix = [&](const double* src, int n, int ld, double** out) -> int {
    void* d = nullptr;
    SC_HIP(h, hipMalloc(&d, (size_t)n * ld * sizeof(double)));
    owned.p.push_back(d);
    SC_HIP(h, hipMemcpyAsync(d, nans.data(), (size_t)n * ld * sizeof(double),
                             hipMemcpyHostToDevice, s));
    *out = reinterpret_cast<double*>(d);
    if (src) SC_TRY(h2d_matrix(h, src, n, n, *out, ld));  // (same stream: after the fill)
    return SC_OK;
  };
  GemmPairItem gm[kGroupMax];
  for (int z = 0; z < count; ++z) {
    const int n = ns[z];
    if (n == 0) continue;
    const int ld = matrix_ld(n);
    double *a = nullptr, *b = nullptr, *add = nullptr, *c = nullptr;
    SC_TRY(device_matrix(As[z], n, ld, &a));
    if (Bs && Bs[z]) SC_TRY(device_matrix(Bs[z], n, ld, &b));
    if (epilogue == kEpiAdd) SC_TRY(device_matrix(addends[z], n, ld, &add));
    SC_TRY(device_matrix(nullptr, n, ld, &c));
    SC_TRY(ensure_tilemap(h, n));
    gm[z].A = a;
    gm[z].B = b;
    gm[z].lda = gm[z].ldb = gm[z].ldc = ld;
    gm[z].C = c;
    gm[z].n = n;
    gm[z].tilemap = h->tilemap_cur;
    gm[z].addend = add;
  }
  SC_HIP(h, hipStreamSynchronize(s));  // (`nans` is pageable)
  launch_gemm_nt_pair_group(s, gm, count, epilogue, full != 0);
  SC_TRY(check_last(h, "grouped product launch"));
  for (int z = 0; z < count; ++z)
    if (ns[z] > 0)
      SC_TRY(d2h_matrix(h, gm[z].C, gm[z].ldc, ns[z], gm[z].ldc, outs[z]));
  SC_HIP(h, hipStreamSynchronize(s));
  return SC_OK;
}
