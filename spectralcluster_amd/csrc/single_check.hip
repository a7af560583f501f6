// The single-cluster test (min_clusters = 1; fallback_clusterer.py:127-187) for a group or a wave
// of a batch.  The single call decides on the host: every Lloyd step and every EM pass of
// sc_affinity_gmm_bic is a parameter upload, two launches, a download and a synchronisation
// (callers_api.hip), 40-90 round trips per utterance.  Here the decision of many utterances is
// device work, in two forms chosen by n exactly as the batch's routes are:
//   short  n <= kDenseMax: ONE launch for up to kScShortMax members, a workgroup each.  The
//          entries a_ij, j >= i + offset, go into LDS once; range, Lloyd steps, M-step, EM passes,
//          final pass and both BICs run inside the kernel, one lane advancing the fit between
//          passes (gmm_common.h: sc_task_advance); the statistics come out of the same launch.
//   chain  kDenseMax < n < 4096: launches of (row blocks x slots), a slot = one task of one
//          member (the statistics, the 1-component fit, the 2-component fit: three independent
//          slots per member, up to 3 kGroupMax per launch).  A pass leaves per-row-block
//          partials; the next launch's prologue adds them in block order, advances the slot
//          (M-step or centre update on the device) and block 0 writes the slot's new state to the
//          other of two buffers, so parameters never visit the host.  A finished slot returns at
//          once.  The host enqueues kScChunk launches at a time and reads the slots once per chunk.
// Every sum has a fixed order that depends on the member's n alone: a member's record is the same
// bits whatever shares its launch.  The per-entry arithmetic, the M-step and the stop rules are
// gmm_common.h's -- the single call's.
#include <algorithm>

#include "gmm_common.h"
#include "handle.h"

namespace sc {

namespace {

constexpr int kScShortThreads = 512;
constexpr int kScChainThreads = 256;

// reduction of value q of a pass: 0 sum, 1 min, 2 max
__device__ __forceinline__ int sc_reduce_op(int kind, int q) {
  if (kind == kScRange) return q == 0 ? 1 : q == 1 ? 2 : 0;
  if (kind == kScStatsA) return q < 2 ? 1 : 0;
  return 0;
}
__device__ __forceinline__ double sc_combine(double a, double b, int op) {
  if (op == 0) return a + b;
  if (op == 1) return b < a ? b : a;
  return b > a ? b : a;
}
__device__ __forceinline__ void sc_acc_init(int kind, double (&acc)[8]) {
  const double inf = __builtin_huge_val();
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = 0.0;
  if (kind == kScRange) {
    acc[0] = inf;
    acc[1] = -inf;
  } else if (kind == kScStatsA) {
    acc[0] = acc[1] = inf;
  }
}
// one entry of the mixture's passes (kScRange .. kScFinal)
__device__ __forceinline__ void sc_fit_entry(double y, int kind, int components,
                                             const GmmCoef& coef, double (&acc)[8]) {
  if (kind == kScRange) {
    gmm_range_entry(y, acc[0], acc[1]);
  } else {
    gmm_entry(y, components, (kind == kScLloyd || kind == kScLabel) ? 0 : 1, coef,
              reinterpret_cast<double(&)[7]>(acc));
  }
}
// one cell (i, j) of the statistics' passes
__device__ __forceinline__ void sc_stats_cell(double v, int i, int j, int kind, double mean,
                                              double (&acc)[8]) {
  if (kind == kScStatsA) {
    stats_entry(v, acc[0], acc[2]);
    if (j == i + 1) acc[1] = v < acc[1] ? v : acc[1];
  } else {
    stats_dev_entry(v, mean, acc[3]);
  }
}
// The workgroup's value of acc[0..8) -> s_sum[0..8): butterflies inside a wavefront, then the
// wavefronts in order.  NW wavefronts; s_w holds NW x 8 doubles.
template <int NW>
__device__ __forceinline__ void sc_block_reduce(double (&acc)[8], int kind, double* s_w,
                                                double* s_sum) {
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    const int op = sc_reduce_op(kind, q);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) acc[q] = sc_combine(acc[q], __shfl_xor(acc[q], o), op);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) s_w[wave * 8 + q] = acc[q];
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int op = sc_reduce_op(kind, threadIdx.x);
    double v = s_w[threadIdx.x];
    for (int w = 1; w < NW; ++w) v = sc_combine(v, s_w[w * 8 + threadIdx.x], op);
    s_sum[threadIdx.x] = v;
  }
  __syncthreads();
}

// ---- short form ---------------------------------------------------------------------------
// rec: 10 doubles per member {min, neighbour min, mean, std, bic1, bic2, lloyd steps, em steps,
// verdict, 0}
__global__ __launch_bounds__(kScShortThreads) void k_single_short(const ScShortArgs a) {
  extern __shared__ double s_y[];  // the entries of the mixture, row after row
  __shared__ ScSlot s_slot;
  __shared__ double s_w[(kScShortThreads / 64) * 8], s_sum[8];
  const ScItem& item = a.it[blockIdx.x];
  const int n = item.n, ld = item.ld, offset = item.offset, tid = threadIdx.x;
  const double* A = item.a;
  double* rec = a.rec + (size_t)blockIdx.x * 10;
  const int m = n - offset;  // entries of row i: m - i
  const int entries = a.gmm ? m * (m + 1) / 2 : 0;
  if (a.gmm) {
    int at = 0;
    for (int i = 0; i < m; ++i) {
      for (int j = i + offset + tid; j < n; j += kScShortThreads)
        s_y[at + j - i - offset] = A[(size_t)i * ld + j];
      at += m - i;
    }
  }
  const double count = (double)m * ((double)m + 1.0) / 2.0, cells = (double)n * (double)n;
  // the statistics first, then the two fits: each a sequence of passes one lane advances
  for (int round = 0; round < (a.gmm ? 3 : 1); ++round) {
    const int task = round == 0 ? kScStats : round == 1 ? kScFit1 : kScFit2;
    __syncthreads();
    if (tid == 0) s_slot = sc_slot_init();
    if (tid < 8) s_sum[tid] = 0.0;
    __syncthreads();
    for (;;) {
      if (tid == 0) sc_task_advance(s_slot, task, s_sum, count, cells);
      __syncthreads();
      const int kind = s_slot.kind;
      if (kind == kScDone) break;
      double acc[8];
      sc_acc_init(kind, acc);
      if (task == kScStats) {
        const double mean = s_slot.params[1];
        for (int c = tid; c < n * n; c += kScShortThreads) {
          const int i = c / n, j = c - i * n;
          sc_stats_cell(A[(size_t)i * ld + j], i, j, kind, mean, acc);
        }
      } else {
        const int components = task == kScFit2 ? 2 : 1;
        const GmmCoef coef = gmm_coef(s_slot.params, components);
        for (int e = tid; e < entries; e += kScShortThreads)
          sc_fit_entry(s_y[e], kind, components, coef, acc);
      }
      sc_block_reduce<kScShortThreads / 64>(acc, kind, s_w, s_sum);
    }
    if (tid == 0) {
      if (task == kScStats) {
        for (int q = 0; q < 4; ++q) rec[q] = s_slot.out[q];
        for (int q = 4; q < 10; ++q) rec[q] = 0.0;
      } else if (task == kScFit1) {
        rec[4] = s_slot.out[0];
      } else {
        rec[5] = s_slot.out[0];
        rec[6] = (double)s_slot.lloyd_steps;
        rec[7] = (double)s_slot.em_steps;
      }
    }
  }
  if (tid == 0) rec[8] = (double)sc_single_verdict(rec, a.condition, a.threshold);
}

// ---- chain form -----------------------------------------------------------------------------
// Launch t reads the slots and partials of buffer t & 1 and writes those of the other one.
__global__ __launch_bounds__(kScChainThreads) void k_single_chain(const ScChainArgs a, int t) {
  __shared__ ScSlot s_slot;
  __shared__ double s_stage[256 * 8];
  __shared__ double s_w[(kScChainThreads / 64) * 8], s_sum[8];
  const int y = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
  const ScItem& item = a.it[y];
  const int n = item.n, ld = item.ld, offset = item.offset, task = item.task;
  const int G = (n + kScRowsPerBlock - 1) / kScRowsPerBlock;  // (<= 256: n < 4096)
  if (blk >= G) return;
  const int cur = t & 1;
  const ScSlot* from = a.slots + (size_t)cur * a.nslots + y;
  ScSlot* to = a.slots + (size_t)(cur ^ 1) * a.nslots + y;
  const double* pc = a.partial + ((size_t)cur * a.nslots + y) * a.gmax * 8;
  double* pn = a.partial + ((size_t)(cur ^ 1) * a.nslots + y) * a.gmax * 8;
  if (tid == 0) s_slot = *from;
  __syncthreads();
  if (s_slot.done) {  // (kept alive in both buffers: the host reads the one written last)
    if (blk == 0 && tid == 0) *to = s_slot;
    return;
  }
  // prologue: the row blocks' partials of the pass before, added in block order
  const int before = s_slot.kind;
  if (before != kScInit) {
    for (int idx = tid; idx < G * 8; idx += kScChainThreads) s_stage[idx] = pc[idx];
    __syncthreads();
    if (tid < 8) {
      const int op = sc_reduce_op(before, tid);
      double v = s_stage[tid];
      for (int g = 1; g < G; ++g) v = sc_combine(v, s_stage[g * 8 + tid], op);
      s_sum[tid] = v;
    }
  } else if (tid < 8) {
    s_sum[tid] = 0.0;
  }
  __syncthreads();
  const int m = n - offset;
  if (tid == 0) {
    sc_task_advance(s_slot, task, s_sum, (double)m * ((double)m + 1.0) / 2.0,
                    (double)n * (double)n);
    if (blk == 0) *to = s_slot;
  }
  __syncthreads();
  const int kind = s_slot.kind;
  if (kind == kScDone) return;
  // this block's rows of the pass: a wavefront per row, rows dealt round-robin to the wavefronts
  double acc[8];
  sc_acc_init(kind, acc);
  const int lane = tid & 63, wave = tid >> 6;
  const int r0 = blk * kScRowsPerBlock, r1 = min(n, r0 + kScRowsPerBlock);
  if (task == kScStats) {
    const double mean = s_slot.params[1];
    for (int i = r0 + wave; i < r1; i += kScChainThreads / 64)
      for (int j = lane; j < n; j += 64) sc_stats_cell(item.a[(size_t)i * ld + j], i, j, kind, mean, acc);
  } else {
    const int components = task == kScFit2 ? 2 : 1;
    const GmmCoef coef = gmm_coef(s_slot.params, components);
    for (int i = r0 + wave; i < r1; i += kScChainThreads / 64)
      for (int j = i + offset + lane; j < n; j += 64)
        sc_fit_entry(item.a[(size_t)i * ld + j], kind, components, coef, acc);
  }
  sc_block_reduce<kScChainThreads / 64>(acc, kind, s_w, s_sum);
  if (tid < 8) pn[(size_t)blk * 8 + tid] = s_sum[tid];
}

}  // namespace

void launch_single_short(hipStream_t s, const ScShortArgs& a, int count, size_t lds_bytes) {
  SC_OPT_IN_LDS(k_single_short, kScShortLds);
  hipLaunchKernelGGL(k_single_short, dim3(count), dim3(kScShortThreads), lds_bytes, s, a);
}
void launch_single_chain(hipStream_t s, const ScChainArgs& a, int t0, int passes) {
  for (int t = t0; t < t0 + passes; ++t)
    hipLaunchKernelGGL(k_single_chain, dim3(a.gmax, a.nslots), dim3(kScChainThreads), 0, s, a, t);
}

}  // namespace sc

// ------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------
namespace {

// the handle's staging for records and slots: device + pinned twin
int ensure_single_staging(sc_handle h) {
  const size_t bytes = std::max((size_t)kScShortMax * 10 * sizeof(double),
                                (size_t)2 * kScChainSlots * sizeof(ScSlot));
  SC_TRY(grow(h, h->sck_rec, (size_t)kScShortMax * 10 * sizeof(double)));
  SC_TRY(grow(h, h->sck_slots, (size_t)2 * kScChainSlots * sizeof(ScSlot)));
  if (!h->h_sck) SC_HIP(h, hipHostMalloc(&h->h_sck, bytes));
  return SC_OK;
}

const char* kOffsetMessage =
    "single_cluster_affinity_diagonal_offset must be significantly smaller than affinity matrix "
    "dimension";

}  // namespace

int single_check_wave(sc_handle lead, hipStream_t s, const SingleMember* ms, int count,
                      const sc_single_check* opt, double* values, int32_t* single) {
  SC_TRY(ensure_single_staging(lead));
  const bool gmm = opt->condition == SC_SINGLE_GMM_BIC;
  for (int at = 0; at < count; at += kScShortMax) {
    const int c = std::min(kScShortMax, count - at);
    ScShortArgs a;
    memset(&a, 0, sizeof(a));
    size_t lds = 0;
    for (int z = 0; z < c; ++z) {
      const SingleMember& mz = ms[at + z];
      if (mz.n < 1 || mz.n > kDenseMax)
        return fail(lead, SC_ERR_INVALID, "single check: a short member outside 1..128 rows");
      a.it[z] = ScItem{mz.a, mz.n, mz.ld, opt->diagonal_offset, 0};
      const size_t m = gmm ? (size_t)(mz.n - opt->diagonal_offset) : 0;
      lds = std::max(lds, m * (m + 1) / 2 * sizeof(double));
    }
    if (lds > kScShortLds) return fail(lead, SC_ERR_INVALID, "single check: LDS budget");
    a.rec = ptr<double>(lead->sck_rec);
    a.gmm = gmm ? 1 : 0;
    a.condition = opt->condition;
    a.threshold = opt->threshold;
    launch_single_short(s, a, c, lds);
    SC_TRY(check_last(lead, "single-cluster test launch"));
    double* rec = static_cast<double*>(lead->h_sck);
    SC_HIP(lead, hipMemcpyAsync(rec, lead->sck_rec.p, (size_t)c * 10 * sizeof(double),
                                hipMemcpyDeviceToHost, s));
    SC_HIP(lead, hipStreamSynchronize(s));
    for (int z = 0; z < c; ++z) {
      if (values) memcpy(values + (size_t)(at + z) * 8, rec + (size_t)z * 10, 8 * sizeof(double));
      single[at + z] = rec[(size_t)z * 10 + 8] != 0.0;
    }
  }
  return SC_OK;
}

int single_check_group(sc_handle lead, hipStream_t s, const SingleMember* ms, int count,
                       const sc_single_check* opt, double* values, int32_t* single) {
  if (count < 1 || count > kGroupMax)
    return fail(lead, SC_ERR_INVALID, "single check: a group holds 1..16 members");
  SC_TRY(ensure_single_staging(lead));
  const bool gmm = opt->condition == SC_SINGLE_GMM_BIC;
  // slots: member z's statistics, and with the mixture condition its two fits beside them
  const int per = gmm ? 3 : 1;
  static const int tasks[3] = {kScStats, kScFit1, kScFit2};
  ScChainArgs a;
  memset(&a, 0, sizeof(a));
  a.nslots = per * count;
  int nmax = 0;
  for (int z = 0; z < count; ++z) {
    if (ms[z].n <= kDenseMax || ms[z].n >= kScChainMaxN)
      return fail(lead, SC_ERR_INVALID, "single check: a chain member outside 129..4095 rows");
    nmax = std::max(nmax, ms[z].n);
    for (int q = 0; q < per; ++q)
      a.it[per * z + q] = ScItem{ms[z].a, ms[z].n, ms[z].ld, opt->diagonal_offset, tasks[q]};
  }
  a.gmax = (nmax + kScRowsPerBlock - 1) / kScRowsPerBlock;
  SC_TRY(grow(lead, lead->sck_part, (size_t)2 * a.nslots * a.gmax * 8 * sizeof(double)));
  a.slots = ptr<ScSlot>(lead->sck_slots);
  a.partial = ptr<double>(lead->sck_part);
  ScSlot* hs = static_cast<ScSlot*>(lead->h_sck);
  for (int q = 0; q < a.nslots; ++q) hs[q] = sc_slot_init();
  SC_HIP(lead, hipMemcpyAsync(a.slots, hs, (size_t)a.nslots * sizeof(ScSlot),
                              hipMemcpyHostToDevice, s));
  // the statistics: pass A, pass B and the launch that takes B's partials -- one chunk
  const int chunk = gmm ? kScChunk : 3;
  const int cap = kScLloydCap + kScEmCap + 8 + chunk;
  for (int t = 0;; t += chunk) {
    launch_single_chain(s, a, t, chunk);
    SC_TRY(check_last(lead, "single-cluster test launch"));
    SC_HIP(lead, hipMemcpyAsync(hs, a.slots + (size_t)((t + chunk) & 1) * a.nslots,
                                (size_t)a.nslots * sizeof(ScSlot), hipMemcpyDeviceToHost, s));
    SC_HIP(lead, hipStreamSynchronize(s));
    bool all = true;
    for (int q = 0; q < a.nslots; ++q) all = all && hs[q].done;
    if (all) break;
    if (t > cap) return fail(lead, SC_ERR_HIP, "single-cluster test did not reach its stop rule");
  }
  for (int z = 0; z < count; ++z) {
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int q = 0; q < 4; ++q) v[q] = hs[per * z].out[q];
    if (gmm) {
      v[4] = hs[per * z + 1].out[0];
      v[5] = hs[per * z + 2].out[0];
      v[6] = (double)hs[per * z + 2].lloyd_steps;
      v[7] = (double)hs[per * z + 2].em_steps;
    }
    if (values) memcpy(values + (size_t)z * 8, v, sizeof(v));
    single[z] = sc_single_verdict(v, opt->condition, opt->threshold);
  }
  return SC_OK;
}

int validate_single_check(sc_handle h, const sc_single_check* opt) {
  if (!opt) return fail(h, SC_ERR_INVALID, "single check is NULL");
  if (opt->condition < SC_SINGLE_GMM_BIC || opt->condition > SC_SINGLE_AFFINITY_STD)
    return fail(h, SC_ERR_UNSUPPORTED,
                "single_cluster_condition must be one of the four affinity conditions");
  return SC_OK;
}

int check_single_offset(sc_handle h, const sc_single_check* opt, int n, int index) {
  if (opt->condition != SC_SINGLE_GMM_BIC) return SC_OK;
  if (opt->diagonal_offset < 0 || opt->diagonal_offset >= n - 1)
    return fail(h, SC_ERR_INVALID, std::string(kOffsetMessage) + " (utterance " +
                                       std::to_string(index) + ")");
  return SC_OK;
}

// The decision on the affinity resident in h (any n: the single call's kernels)
int single_check_resident(sc_handle h, const sc_single_check* opt, double* values,
                          int32_t* single) {
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  SC_TRY(affinity_stats_impl(h, v));
  if (opt->condition == SC_SINGLE_GMM_BIC)
    SC_TRY(affinity_gmm_bic_impl(h, opt->diagonal_offset, &v[4], &v[5]));
  if (values) memcpy(values, v, sizeof(v));
  *single = sc_single_verdict(v, opt->condition, opt->threshold);
  return SC_OK;
}

extern "C" int sc_single_check_layout(int* check_bytes, int* field_offsets) {
  if (check_bytes) *check_bytes = (int)sizeof(sc_single_check);
  if (field_offsets) {
    field_offsets[0] = (int)offsetof(sc_single_check, condition);
    field_offsets[1] = (int)offsetof(sc_single_check, diagonal_offset);
    field_offsets[2] = (int)offsetof(sc_single_check, threshold);
  }
  return SC_OK;
}

extern "C" int sc_batch_single_check(sc_handle h, const double* const* affinities, const int* ns,
                                     int count, const sc_single_check* opt, double* values,
                                     int32_t* single) {
  if (!h) return SC_ERR_INVALID;
  if (!affinities || !ns || !values || !single || count < 0)
    return fail(h, SC_ERR_INVALID, "NULL argument");
  SC_TRY(validate_single_check(h, opt));
  for (int i = 0; i < count; ++i) {
    if (!affinities[i] || ns[i] < 1) return fail(h, SC_ERR_INVALID, "affinity must be (n, n)");
    SC_TRY(check_single_offset(h, opt, ns[i], i));
  }
  SC_HIP(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  // largest first, as the batch sorts its routes: waves of the short members, groups of the rest
  std::vector<int> shorts, chain, large;
  for (int i = 0; i < count; ++i)
    (ns[i] <= kDenseMax ? shorts : ns[i] < kScChainMaxN ? chain : large).push_back(i);
  auto by_size = [&](int a, int b) { return ns[a] > ns[b]; };
  std::stable_sort(shorts.begin(), shorts.end(), by_size);
  std::stable_sort(chain.begin(), chain.end(), by_size);
  auto run = [&](const std::vector<int>& list, int width, bool wave) -> int {
    for (size_t at = 0; at < list.size(); at += width) {
      const int c = (int)std::min<size_t>(width, list.size() - at);
      size_t cells = 0;
      for (int z = 0; z < c; ++z) cells += (size_t)ns[list[at + z]] * ns[list[at + z]];
      SC_TRY(grow(h, h->sck_mats, cells * sizeof(double)));
      std::vector<SingleMember> ms(c);
      std::vector<double> vals((size_t)c * 8);
      std::vector<int32_t> one(c);
      size_t off = 0;
      for (int z = 0; z < c; ++z) {
        const int i = list[at + z], n = ns[i];
        double* dst = ptr<double>(h->sck_mats) + off;
        SC_HIP(h, hipMemcpyAsync(dst, affinities[i], (size_t)n * n * sizeof(double),
                                 hipMemcpyHostToDevice, s));
        ms[z] = SingleMember{dst, n, n};
        off += (size_t)n * n;
      }
      SC_TRY(wave ? single_check_wave(h, s, ms.data(), c, opt, vals.data(), one.data())
                  : single_check_group(h, s, ms.data(), c, opt, vals.data(), one.data()));
      for (int z = 0; z < c; ++z) {
        memcpy(values + (size_t)list[at + z] * 8, vals.data() + (size_t)z * 8, 8 * sizeof(double));
        single[list[at + z]] = one[z];
      }
    }
    return SC_OK;
  };
  // (every argument has been checked above; from here on only a HIP error ends the call)
  SC_TRY(run(shorts, kScShortMax, true));
  SC_TRY(run(chain, kGroupMax, false));
  for (int i : large) {  // n >= 4096: the single call's decision on this handle
    SC_TRY(sc_set_affinity(h, affinities[i], ns[i]));
    SC_TRY(single_check_resident(h, opt, values + (size_t)i * 8, single + i));
  }
  return SC_OK;
}
