// The arithmetic of the single-cluster decisions (fallback_clusterer.py:137-173), stated once:
// per-entry bodies of the affinity statistics and of the 1-D Gaussian mixture passes, sklearn's
// M-step, and the step from one pass of a fit to the next.  fallback.hip (the single call, driven
// by the host: callers_api.hip) and single_check.hip (a group or wave of a batch, driven on the
// device) both include it.
#ifndef SPECTRALCLUSTER_AMD_GMM_COMMON_H_
#define SPECTRALCLUSTER_AMD_GMM_COMMON_H_

#include <hip/hip_runtime.h>

#include <cmath>

namespace sc {

// ---- per-entry bodies ---------------------------------------------------------------------
// what a pass under params = {w0, mu0, var0, w1, mu1, var1} needs of them
struct GmmCoef {
  double mu0, v0, lw0, mu1, v1, lw1;
};
__device__ __forceinline__ GmmCoef gmm_coef(const double* params, int components) {
  const double kLog2Pi = 1.8378770664093453;
  const double w0 = params[0], w1 = params[3];
  GmmCoef c;
  c.mu0 = params[1];
  c.v0 = params[2];
  c.mu1 = params[4];
  c.v1 = params[5];
  c.lw0 = log(w0) - 0.5 * (kLog2Pi + log(c.v0));
  c.lw1 = components > 1 ? log(w1) - 0.5 * (kLog2Pi + log(c.v1)) : 0.0;
  return c;
}
// mode 0: hard assignment to the nearer of the centres mu0, mu1 (ties: the first), acc[6] += the
//         squared distance (inertia)
// mode 1: responsibilities under the mixture, acc[6] += the entry's log-likelihood
// acc[0..5] += {r0, r0 y, r0 y^2, r1, r1 y, r1 y^2}
__device__ __forceinline__ void gmm_entry(double y, int components, int mode, const GmmCoef& c,
                                          double (&acc)[7]) {
  double r0 = 1.0, r1 = 0.0, extra;
  if (mode == 0) {
    const double d0 = (y - c.mu0) * (y - c.mu0), d1 = (y - c.mu1) * (y - c.mu1);
    if (d1 < d0) {  // ties go to the first centre (argmin)
      r0 = 0.0;
      r1 = 1.0;
    }
    extra = d1 < d0 ? d1 : d0;
  } else {
    const double l0 = c.lw0 - 0.5 * (y - c.mu0) * (y - c.mu0) / c.v0;
    if (components > 1) {
      const double l1 = c.lw1 - 0.5 * (y - c.mu1) * (y - c.mu1) / c.v1;
      const double mx = l0 > l1 ? l0 : l1;
      const double lse = mx + log(exp(l0 - mx) + exp(l1 - mx));
      r0 = exp(l0 - lse);
      r1 = exp(l1 - lse);
      extra = lse;
    } else {
      extra = l0;
    }
  }
  acc[0] += r0;
  acc[1] += r0 * y;
  acc[2] += r0 * y * y;
  acc[3] += r1;
  acc[4] += r1 * y;
  acc[5] += r1 * y * y;
  acc[6] += extra;
}
__device__ __forceinline__ void gmm_range_entry(double y, double& mn, double& mx) {
  mn = y < mn ? y : mn;
  mx = y > mx ? y : mx;
}
// first pass of the statistics: running minimum and sum (NaN never wins the minimum: np.min
// would return NaN; affinities are finite)
__device__ __forceinline__ void stats_entry(double v, double& mn, double& sum) {
  mn = v < mn ? v : mn;
  sum += v;
}
// second pass of np.std
__device__ __forceinline__ void stats_dev_entry(double v, double mu, double& acc) {
  const double dv = v - mu;
  acc += dv * dv;
}

// ---- the M-step -----------------------------------------------------------------------------
// sklearn's _estimate_gaussian_parameters from the sums of a pass (reg_covar 1e-6, tiny =
// 10 eps, weights renormalised); `count`: the number of entries
__host__ __device__ inline void gmm_m_step(const double* sums, int components, double count,
                                           double* params) {
  const double reg = 1e-6, tiny = 10.0 * 2.220446049250313e-16;
  double wsum = 0.0;
  for (int c = 0; c < components; ++c) {
    const double nk = sums[3 * c] + tiny;
    const double mu = sums[3 * c + 1] / nk;
    const double var = (sums[3 * c + 2] - 2.0 * mu * sums[3 * c + 1] + mu * mu * sums[3 * c]) / nk;
    params[3 * c] = nk / count;
    params[3 * c + 1] = mu;
    params[3 * c + 2] = var + reg;
    wsum += params[3 * c];
  }
  for (int c = 0; c < components; ++c) params[3 * c] /= wsum;
}

// ---- a fit as a sequence of passes ----------------------------------------------------------
// The single call's host loop (callers_api.hip: sc_affinity_gmm_bic) as a state that one lane
// advances between passes.  `kind` names the pass whose sums are in; sc_task_advance() consumes
// them and leaves the kind and the parameters of the next pass.
enum ScTask { kScFit1 = 0, kScFit2 = 1, kScStats = 2 };
enum ScPassKind {
  kScInit = 0,   // nothing has run
  kScRange,      // min / max of the entries: the 2-means start
  kScLloyd,      // a Lloyd step (gmm_entry mode 0)
  kScLabel,      // the final hard labels (mode 0): their sums are the first M-step's
  kScMoments,    // the 1-component fit's plain moments (mode 1 under {1, 0, 1})
  kScEm,         // an EM pass (mode 1)
  kScFinal,      // the pass the BIC is computed from (mode 1)
  kScStatsA,     // min, neighbour min, sum over the whole matrix
  kScStatsB,     // sum of squared deviations from the mean
  kScDone
};
constexpr int kScLloydCap = 300, kScEmCap = 100;
struct ScSlot {
  double params[6];
  double prev;    // inertia of the Lloyd step before / lower bound of the EM pass before
  double out[4];  // a fit: out[0] = BIC; the statistics: {min, neighbour min, mean, std}
  int kind, it;
  int lloyd_steps, em_steps;  // passes of the Lloyd loop / of the EM loop
  int done, pad;
};

__host__ __device__ inline ScSlot sc_slot_init() {
  ScSlot s;
  for (int i = 0; i < 6; ++i) s.params[i] = 0.0;
  s.prev = 0.0;
  for (int i = 0; i < 4; ++i) s.out[i] = 0.0;
  s.kind = kScInit;
  s.it = s.lloyd_steps = s.em_steps = s.done = s.pad = 0;
  return s;
}

// `sums`: what the pass s.kind left ({n0, s0, q0, n1, s1, q1, inertia | loglik}; kScRange:
// {min, max}; kScStatsA: {min, neighbour min, sum}; kScStatsB: [3] = sum of squares);
// `count`: entries of the mixture; `cells`: n * n
__device__ __forceinline__ void sc_task_advance(ScSlot& s, int task, const double* sums,
                                                double count, double cells) {
  const int components = task == kScFit2 ? 2 : 1;
  auto start_em = [&]() {
    gmm_m_step(sums, components, count, s.params);
    s.kind = kScEm;
    s.it = 0;
    s.prev = -__builtin_huge_val();
  };
  switch (s.kind) {
    case kScInit:
      s.params[0] = 1.0;
      s.params[1] = 0.0;
      s.params[2] = 1.0;
      s.params[3] = 0.0;
      s.params[4] = 0.0;
      s.params[5] = 1.0;
      s.kind = task == kScFit1 ? kScMoments : task == kScFit2 ? kScRange : kScStatsA;
      break;
    case kScRange:  // 2-means start from the extremes
      s.params[1] = sums[0];
      s.params[4] = sums[1];
      s.prev = -1.0;
      s.it = 0;
      s.kind = kScLloyd;
      break;
    case kScLloyd: {  // ... Lloyd steps until the inertia stops moving
      const double inertia = sums[6];
      if (sums[0] > 0.0) s.params[1] = sums[1] / sums[0];
      if (sums[3] > 0.0) s.params[4] = sums[4] / sums[3];
      s.lloyd_steps = s.it + 1;
      if (inertia == s.prev || s.it + 1 >= kScLloydCap) {
        s.kind = kScLabel;
      } else {
        s.prev = inertia;
        ++s.it;
      }
      break;
    }
    case kScLabel:    // responsibilities = the final hard labels
    case kScMoments:  // r0 = 1 everywhere: plain moments
      start_em();
      break;
    case kScEm: {  // E-step under params (+ the sums of the M-step)
      const double lower_bound = sums[6] / count;
      gmm_m_step(sums, components, count, s.params);
      s.em_steps = s.it + 1;
      if (fabs(lower_bound - s.prev) < 1e-3 || s.it + 1 >= kScEmCap) {
        s.kind = kScFinal;
      } else {
        s.prev = lower_bound;
        ++s.it;
      }
      break;
    }
    case kScFinal: {
      const double n_params = components == 1 ? 2.0 : 5.0;
      s.out[0] = -2.0 * sums[6] + n_params * log(count);
      s.kind = kScDone;
      s.done = 1;
      break;
    }
    case kScStatsA:
      s.out[0] = sums[0];
      s.out[1] = sums[1];
      s.out[2] = sums[2] / cells;
      s.params[1] = s.out[2];
      s.kind = kScStatsB;
      break;
    case kScStatsB:
      s.out[3] = sqrt(sums[3] / cells);
      s.kind = kScDone;
      s.done = 1;
      break;
    default:
      s.done = 1;
      break;
  }
}

// The verdict of a member from its record {min, neighbour min, mean, std, bic1, bic2, ...}
// (fallback_clusterer.py:137-173; condition: SingleClusterCondition)
__host__ __device__ inline int sc_single_verdict(const double* v, int condition, double threshold) {
  switch (condition) {
    case 1: return v[4] < v[5];      // AffinityGmmBic
    case 2: return v[0] > threshold;  // AllAffinity
    case 3: return v[1] > threshold;  // NeighborAffinity
    default: return v[3] < threshold;  // AffinityStd
  }
}

}  // namespace sc

#endif  // SPECTRALCLUSTER_AMD_GMM_COMMON_H_
