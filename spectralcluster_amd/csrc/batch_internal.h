// What batch_group.hip (the grouped batch), batch_sweep.hip (an AutoTune level as a group),
// batch_autotune.hip (a batch of AutoTune searches) and stage_front.hip (the test hook) share.
// Plain declarations, as in handle.h; each function is defined in the file named above its block.
#ifndef SPECTRALCLUSTER_AMD_BATCH_INTERNAL_H_
#define SPECTRALCLUSTER_AMD_BATCH_INTERNAL_H_

#include "handle.h"

struct Member {
  int index = -1;        // utterance
  sc_handle h = nullptr;
  FrontResult front;      // (front.free_op: matrix-free Diffuse, front.matrix is A)
  int state = 0;         // 0 in the group, 1 single-call path, 2 done
  int k = 0;
  const GroupEigMember* eig = nullptr;  // what the group's eigensolver left for it
};

// What a constrained batch carries (sc_predict_batch_constraints): per utterance one constraint
// that is the band of its ConstraintMatrix (kind 2: n_i - 1 values), a list of directed entries
// (kind 3) or nothing (kind 0); host memory, validated before the batch starts.
struct Bands {
  const sc_constraint_desc* cons = nullptr;  // nullptr: the batch carries no constraints
  // per utterance of kind 3: vals | rows | cols as Cpairs holds them (the upload's source, alive
  // for the whole call) and whether the list is symmetric
  const std::vector<double>* packed = nullptr;
  const char* pairs_symmetric = nullptr;
  int kmax = 0;        // the largest entry list: what a member arena reserves
  bool chain = false;  // ConstraintPropagation before refinement: the grouped Neumann chain
  int ncp = 0;         // cp[] work matrices a member arena holds for the configured operator
  // sc_predict_batch_affinities: the batch's arrays are (n, n) affinities the callers hold, not
  // embeddings -- the grouped ingest of a front replaces the rows' upload and the affinity GEMM
  bool affinities = false;
  // sc_predict_batch_constraint_arrays: dense[i].data != nullptr -- utterance i carries a dense
  // (n_i, n_i) constraint as a described source (its cons[i].kind is 0); nullptr: no member does
  const sc_array* dense = nullptr;
  bool is_dense(int i) const { return dense && dense[i].data; }
  bool has(int i) const { return (cons && cons[i].kind != 0) || is_dense(i); }
  const double* band(int i) const { return cons && cons[i].kind == 2 ? cons[i].band : nullptr; }
  bool pairs(int i) const { return cons && cons[i].kind == 3; }
};

// What a min_clusters = 1 batch carries (sc_predict_batch_single): the single-cluster test every
// utterance's raw affinity takes before its eigensolver, and where the verdicts go (one per
// utterance, zeroed by predict_batch_core; may be null).
struct SingleCheck {
  const sc_single_check* opt = nullptr;
  int32_t* single = nullptr;
};

// What sc_eig_ncluster_sweep decides before its rounds: which of the two sequences it groups,
// whether the level runs as a group at all, and the route of its Diffuse.
struct SweepPlan {
  bool icassp = false, thr_sym_only = false, grouped = false;
  bool free_route = false, amax_from_cut = false;
  // n <= kDenseMax: the level's values as (matrix, p) pairs -- one front launch and ONE Jacobi
  // launch for up to kShortWidth of them (sweep_short_level)
  bool short_level = false;
};

// What every value of a short level shares (sweep_short_shared)
struct ShortShared {
  const double* src = nullptr;   // the matrix every value thresholds
  const double* crop = nullptr;  // CropDiagonal's value vector (fused form only)
  int crop_source = 0;
};

// d <= kShortWaveMaxD: a single call of n <= 128 runs its affinity product as whole-K tiles
// (gemm_f64.hip launch_variant: "if (K <= 512 && full == 0) ksplit = 1"), which is what the
// grouped product computes -- the wave front's bits are then the single call's.  The Diffuse
// product has K = n <= 128.
constexpr int kShortWaveMaxD = 512;

// ---- batch_group.hip ---------------------------------------------------------------------
// Member arena z of `lead` (created on demand); `arenas`: the list to use (default: lead->gslots)
int group_slot(sc_handle lead, int z, sc_handle* out, std::vector<sc_handle_s*>* arenas = nullptr);
int ensure_bank_stream(sc_handle h, int b);
int ensure_seed_table(sc_handle lead);
int reserve_bank_arenas(sc_handle h, const sc_config* cfg, const EigRequest& rq, int bank,
                        int positions, int largest, int d, const Bands* bands);
int upload_group_blur_weights(sc_handle h, const sc_config* cfg);

// Launch descriptors of a member arena whose problem is resident (n, d, pitches: the arena's).
// Every front builds them here; what a route passes differently is an assignment behind the call.
enum FrontParts {
  kFrontRows = 1,     // X, Xn, ldx, d, symflag: what the row normalisation reads and writes
  kFrontSource = 2,   // A0, cropval, B1, rmpart: the arena's own affinity and blurred matrix
  kFrontRefined = 4,  // B2, cut, rowmax, rowsum, cvec, pvec, tvec: what the refinement leaves
};
// (n, ldn and flags always; every other field stays zero; blur_cols is the caller's)
FrontItem front_item(sc_handle h, int parts);
// Xn Xn^T -> A0 with the per-tile row maxima off the diagonal in statp; rowmax stays null
GemmGroupItem affinity_item(sc_handle h);
// B2 B2^T -> B1 with per-tile row maxima and sums in statp; `reduced_stats`: the launch folds them
// into the arena's rowmax / rowsum (else both stay null: a kernel of the caller's reads statp)
GemmGroupItem diffuse_item(sc_handle h, bool reduced_stats);
ShortWaveItem short_wave_item(sc_handle h);

bool grouped_front_covers(const sc_config* cfg);
bool short_wave_covers(const sc_config* cfg, ShortWaveOps* ops);
int enqueue_front_grouped(sc_handle lead, const sc_array* xs, const int* ns, int d,
                          const sc_config* cfg, sc_diag* diags, const int* idx, int count,
                          int slot0, Member* mb, int bank);
int enqueue_front_short_wave(sc_handle lead, const sc_array* xs, const int* ns, int d,
                             const sc_config* cfg, sc_diag* diags, const int* idx, int count,
                             int slot0, Member* mb, int bank, const ShortWaveOps& ops);
int cluster_members(sc_handle lead, const int* ns, const sc_config* cfg, int64_t* const* labels,
                    sc_diag* diags, Member* mb, const int* zs, int nz, const EigRequest& rq,
                    int eig_path, int route, int* clustered);

// The lanes of a batch: leads[0] = h, leads[1..lanes) the handles of h->glanes (created on
// demand; `what` names the batch in the error text), each with h's blur weights and route report.
int ensure_lanes(sc_handle h, int lanes, const char* what, sc_handle* leads);
// The cost model the lanes are balanced by (microseconds of an utterance of n rows, roughly)
inline double unit_cost(int n) { return 60.0 + 3.5e-5 * (double)n * n; }
// `items` in the order given, each (load: cost(item)) to the least loaded lane, ties to the lower
template <typename Cost>
void deal_least_loaded(const std::vector<int>& items, Cost cost, int lanes,
                       std::vector<int>* lists) {
  double load[kGroupLanes] = {0.0};
  for (int item : items) {
    int best = 0;
    for (int l = 1; l < lanes; ++l)
      if (load[l] < load[best]) best = l;
    lists[best].push_back(item);
    load[best] += cost(item);
  }
}
// Member arenas (gslots) that hold a quarter of the device do not outlive the call; `always`:
// whatever they hold.  Returns whether they were freed (the leads' sweep_slot is cleared then).
bool release_large_arenas(sc_handle* leads, int lanes, bool always = false);

// ---- batch_sweep.hip ---------------------------------------------------------------------
// Does the configuration name one of the two sequences a sweep groups?  `plan` (may be null):
// icassp / thr_sym_only are set.
bool swept_sequence(const sc_config* cfg, SweepPlan* plan);
SweepPlan sweep_plan(sc_handle h, const sc_config* cfg, int count, const EigRequest& rq);
int sweep_shared_blur(sc_handle h, const sc_config* cfg, const double** crop_out = nullptr,
                      int* crop_source = nullptr);
int sweep_round_members(sc_handle h, const sc_config* cfg, const SweepPlan& plan,
                        const EigRequest& rq, const double* ps, int cnt, FrontItem* fi,
                        GemmGroupItem* dif, GroupEigMember* em, bool* out_of_memory,
                        int slot0 = 0, sc_handle owner = nullptr);
int sweep_round_front(sc_handle h, const sc_config* cfg, const SweepPlan& plan, const double* ps,
                      int cnt, FrontItem* fi, GemmGroupItem* dif, GroupEigMember* em,
                      FrontResult* taken = nullptr);
int sweep_short_shared(sc_handle h, const sc_config* cfg, const SweepPlan& plan, ShortShared* sh);
int short_pairs_launch(sc_handle h, const sc_config* cfg, const SweepPlan& plan,
                       const double* const* srcs, const double* ps, int cnt, const FrontItem* fi,
                       const GemmGroupItem* dif);
int sweep_short_front(sc_handle h, const sc_config* cfg, const SweepPlan& plan,
                      const EigRequest& rq, const ShortShared& sh, const double* ps, int cnt,
                      FrontItem* fi, GemmGroupItem* dif, GroupEigMember* em, bool* out_of_memory);

#endif  // SPECTRALCLUSTER_AMD_BATCH_INTERNAL_H_
