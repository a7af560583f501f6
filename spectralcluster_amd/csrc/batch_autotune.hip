// sc_predict_batch_autotune: a batch in which every utterance is an AutoTune search (the
// Turn-to-Diarize configuration).  Utterances of n <= kDenseMax run in waves of kShortWidth on the
// caller's thread: the levels of all their searches are evaluated together as (utterance, p) pairs
// through the short level of the sweep (batch_sweep.hip: short_pairs_launch), the winners' k-means
// as the grouped batch's lockstep chain (batch_group.hip: cluster_members).  Mid-size utterances
// are dealt to the lanes of the grouped batch, one search after the other on each
// (sc_eig_ncluster_sweep); the rest, and whatever left its route, runs on the caller's handle.
#include <map>
#include <thread>
#include <utility>

#include "batch_internal.h"

namespace {
// One utterance on one handle and stream: the AutoTune branch of SpectralClusterer._predict --
// ingest, the band resident and applied before refinement, the levels through
// sc_eig_ncluster_sweep under the host search, the winner adopted from the last level (a single
// evaluation when it left it), sc_cluster.  No constraint is resident in `h` afterwards.
struct SearchOnHandle {
  sc_handle h;
  const sc_config* cfg;
  const sc_autotune* at;
  std::vector<double> last_ps;  // the values of the level evaluated last
};
int search_level_on_handle(const double* ps, int count, double* ratios, void* user) {
  SearchOnHandle* c = static_cast<SearchOnHandle*>(user);
  std::vector<sc_diag> diags(count);
  const int rc = sc_eig_ncluster_sweep(c->h, c->cfg, ps, count, diags.data());
  if (rc != SC_OK) return rc;
  c->last_ps.assign(ps, ps + count);
  for (int i = 0; i < count; ++i)
    if (sc_host_autotune_ratio(c->at, ps[i], diags[i].max_delta, ratios + i) != SC_OK)
      return SC_ERR_INVALID;
  return SC_OK;
}
int autotune_one(sc_handle h, const sc_array& x, const double* band, const sc_config* cfg,
                 const sc_autotune* at, int64_t* labels, sc_diag* diag, double* best_p,
                 double* last_p) {
  struct NoConstraintLeft {
    sc_handle h;
    ~NoConstraintLeft() { (void)sc_clear_constraint(h); }
  } cleanup{h};
  const int n = (int)x.rows;
  if (band && cfg->constraint_name != SC_CONSTRAINT_NONE)
    SC_TRY(sc_set_constraint_band(h, band, n));
  else
    SC_TRY(sc_clear_constraint(h));
  SC_TRY(ingest_embeddings(h, x, x.location == SC_MEM_HOST));
  SC_TRY(sc_compute_affinity(h));
  if (constraint_active(h, cfg, true)) SC_TRY(sc_apply_constraint(h, cfg));
  SearchOnHandle ctx{h, cfg, at, {}};
  double win = 0.0, last = 0.0;
  int rc = sc_host_autotune_search(at, search_level_on_handle, &ctx, &win, nullptr, &last, nullptr);
  if (rc != SC_OK) {
    if (h->err.empty())
      fail(h, rc, "the AutoTune search has no winner (no level, or no finite ratio)");
    return rc;
  }
  sc_config c = *cfg;
  c.p_percentile = win;
  sc_diag local;
  sc_diag* dg = diag ? diag : &local;
  int index = -1;
  for (int i = 0; i < (int)ctx.last_ps.size(); ++i)
    if (ctx.last_ps[i] == win) index = i;
  if (index < 0 || sc_sweep_adopt(h, &c, index, dg) != SC_OK) SC_TRY(sc_eig_ncluster(h, &c, dg));
  int k = dg->n_clusters_raw;
  if (cfg->min_clusters > 0 && k < cfg->min_clusters) k = cfg->min_clusters;
  SC_TRY(sc_cluster(h, &c, k, labels, dg));
  if (best_p) *best_p = win;
  if (last_p) *last_p = last;
  return SC_OK;
}

// ---- the short route: utterances of n <= kDenseMax in waves, level by level
// The host search is driven by a callback; here the levels of many utterances are evaluated
// together, so a search is REPLAYED: it runs from the entry state on the ratios known so far and
// stops at the first level that needs a value nobody has evaluated -- those values join the wave's
// next launches -- until it runs through.  (A search is a few hundred flops.)
constexpr int kSearchPending = 1;  // (no sc_status is positive)
struct Replay {
  const std::map<double, double>* known;
  std::vector<double> pending;
};
int replay_level(const double* ps, int count, double* ratios, void* user) {
  Replay* r = static_cast<Replay*>(user);
  r->pending.clear();
  for (int i = 0; i < count; ++i) {
    const auto it = r->known->find(ps[i]);
    if (it == r->known->end()) r->pending.push_back(ps[i]);
    else ratios[i] = it->second;
  }
  return r->pending.empty() ? SC_OK : kSearchPending;
}

struct ShortUtterance {
  int index = -1;        // utterance of the batch
  sc_handle h = nullptr;  // its arena: affinity (adjusted by its band), what its values share
  SweepPlan plan;
  ShortShared shared;
  std::map<double, double> ratio;  // proxy per evaluated p_percentile
  std::vector<double> pending;
  bool done = false, left = false;  // `left`: goes through autotune_one on the caller's handle
  double best_p = 0.0, last_p = 0.0;
};

// (utterance, p) pairs in launches of up to kShortWidth: ONE front launch, ONE Jacobi launch each.
// `on_pair(q, em)`: called per solved pair of a launch, q its position in `pairs`.
template <typename F>
int short_pairs_run(sc_handle lead, const sc_config* cfg, const EigRequest& rq,
                    std::vector<ShortUtterance>& us,
                    const std::vector<std::pair<int, double>>& pairs,
                    std::vector<FrontItem>& fi, std::vector<GemmGroupItem>& dif,
                    std::vector<GroupEigMember>& em, F on_launch) {
  // (pairs of one sequence only: a wave's utterances share the configuration, hence the plan)
  for (size_t base = 0; base < pairs.size(); base += kShortWidth) {
    const int cnt = (int)std::min<size_t>(kShortWidth, pairs.size() - base);
    memset(fi.data(), 0, fi.size() * sizeof(FrontItem));
    const double* srcs[kShortWidth];
    double ps[kShortWidth];
    for (int q = 0; q < cnt; ++q) {
      ShortUtterance& u = us[pairs[base + q].first];
      ps[q] = pairs[base + q].second;
      srcs[q] = u.shared.src;
      bool out_of_memory = false;
      const int rc = sweep_round_members(u.h, cfg, u.plan, rq, ps + q, 1, fi.data() + q,
                                         dif.data() + q, em.data() + q, &out_of_memory, q, lead);
      if (rc != SC_OK) return fail(lead, rc, u.h->err);
      if (out_of_memory)
        return fail(lead, SC_ERR_OOM, "a pair arena of the AutoTune batch does not fit");
    }
    SC_TRY(short_pairs_launch(lead, cfg, us[pairs[base].first].plan, srcs, ps, cnt, fi.data(),
                              dif.data()));
    SC_TRY(dense_topk_group(lead, em.data(), cnt));
    SC_TRY(on_launch((int)base, cnt));
  }
  return SC_OK;
}

int autotune_short_wave(sc_handle lead, const sc_array* xs, const double* const* bands,
                        const int* ns, int d, const sc_config* cfg, const sc_autotune* at,
                        const EigRequest& rq, const int* idx, int count, int64_t* const* labels,
                        sc_diag* diags, double* best_p, double* last_p, std::vector<int>* left) {
  hipStream_t s = lead->stream;
  std::vector<ShortUtterance> us(count);
  // ---- fronts per utterance on the member streams: affinity, band, the part its values share
  for (int z = 0; z < count; ++z) {
    ShortUtterance& u = us[z];
    u.index = idx[z];
    SC_TRY(group_slot(lead, z, &u.h, &lead->gshort));
    sc_handle h = u.h;
    h->err.clear();
    int rc = sc_reserve(h, kDenseMax, d);
    const double* band = bands ? bands[u.index] : nullptr;
    if (rc == SC_OK)
      rc = band && cfg->constraint_name != SC_CONSTRAINT_NONE
               ? sc_set_constraint_band(h, band, ns[u.index]) : sc_clear_constraint(h);
    if (rc == SC_OK) rc = ingest_embeddings(h, xs[u.index], false);
    if (rc == SC_OK) rc = sc_compute_affinity(h);
    if (rc == SC_OK && constraint_active(h, cfg, true)) rc = sc_apply_constraint(h, cfg);
    if (rc == SC_OK) {
      u.plan = sweep_plan(h, cfg, 2, rq);
      if (!u.plan.short_level) u.left = u.done = true;  // (a sequence the sweep does not group)
      else rc = sweep_short_shared(h, cfg, u.plan, &u.shared);
    }
    if (rc != SC_OK) return fail(lead, rc, h->err);
    SC_HIP(lead, hipEventRecord(h->sync_ev, h->stream));
    SC_HIP(lead, hipStreamWaitEvent(s, h->sync_ev, 0));
  }
  std::vector<FrontItem> fi(kShortWidth);
  std::vector<GemmGroupItem> dif(kShortWidth);
  std::vector<GroupEigMember> em(kShortWidth);
  // ---- the levels: replay every open search, evaluate what they ask for, again
  for (;;) {
    std::vector<std::pair<int, double>> pairs;
    for (int z = 0; z < count; ++z) {
      ShortUtterance& u = us[z];
      if (u.done) continue;
      Replay replay{&u.ratio, {}};
      const int rc = sc_host_autotune_search(at, replay_level, &replay, &u.best_p, nullptr,
                                             &u.last_p, nullptr);
      if (rc == SC_OK) {
        u.done = true;
      } else if (rc == kSearchPending) {
        for (double p : replay.pending) pairs.emplace_back(z, p);
      } else {
        return fail(lead, rc, "the AutoTune search has no winner (no level, or no finite ratio)");
      }
    }
    if (pairs.empty()) break;
    SC_TRY(short_pairs_run(lead, cfg, rq, us, pairs, fi, dif, em, [&](int base, int cnt) -> int {
      for (int q = 0; q < cnt; ++q) {
        ShortUtterance& u = us[pairs[base + q].first];
        if (em[q].status != 0) {  // the single call states the error
          u.left = u.done = true;
          continue;
        }
        double ratio = 0.0;
        if (sc_host_autotune_ratio(at, pairs[base + q].second, em[q].dc.max_delta, &ratio) != SC_OK)
          return fail(lead, SC_ERR_INVALID, "AutoTune proxy");
        u.ratio[pairs[base + q].second] = ratio;
      }
      return SC_OK;
    }));
  }
  // ---- the winners: their eigenvectors (one pair per utterance), then the lockstep k-means
  std::vector<std::pair<int, double>> winners;
  for (int z = 0; z < count; ++z)
    if (!us[z].left) winners.emplace_back(z, us[z].best_p);
  std::vector<Member> mb(kShortWidth);
  SC_TRY(short_pairs_run(lead, cfg, rq, us, winners, fi, dif, em, [&](int base, int cnt) -> int {
    std::vector<int> zs;
    for (int q = 0; q < cnt; ++q) {
      ShortUtterance& u = us[winners[base + q].first];
      Member& m = mb[q];
      m = Member();
      m.index = u.index;
      m.h = em[q].h;
      m.eig = &em[q];
      m.front.folded_rownorm = u.plan.icassp;
      if (diags) memset(diags + u.index, 0, sizeof(sc_diag));
      zs.push_back(q);
    }
    for (int at0 = 0; at0 < cnt; at0 += kGroupMax)
      SC_TRY(cluster_members(lead, ns, cfg, labels, diags, mb.data(), zs.data() + at0,
                             std::min(kGroupMax, cnt - at0), rq, SC_EIG_PATH_DENSE_JACOBI,
                             SC_BATCH_ROUTE_GROUP_JACOBI, nullptr));
    for (int q = 0; q < cnt; ++q) {
      ShortUtterance& u = us[winners[base + q].first];
      if (mb[q].state != 2) {
        u.left = true;
        continue;
      }
      if (diags && !u.plan.icassp) diags[u.index].diffuse_path = SC_DIFFUSE_PATH_NONE;
      if (best_p) best_p[u.index] = u.best_p;
      if (last_p) last_p[u.index] = u.last_p;
    }
    return SC_OK;
  }));
  for (int z = 0; z < count; ++z)
    if (us[z].left) left->push_back(us[z].index);
  return SC_OK;
}
}  // namespace

extern "C" int sc_predict_batch_autotune(sc_handle h, const sc_array* xs,
                                         const double* const* bands, int count,
                                         const sc_config* cfg, const sc_autotune* at,
                                         int64_t* const* labels, sc_diag* diags, double* best_p,
                                         int group, double* last_p) {
  if (!h) return SC_ERR_INVALID;
  if (!xs || !labels || !at || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  if (group < 2)
    return fail(h, SC_ERR_INVALID, "sc_predict_batch_autotune is the grouped form: group >= 2");
  SC_TRY(validate_config(h, cfg));
  if (at->proxy != SC_AUTOTUNE_PERCENTILE_OVER_NME &&
      at->proxy != SC_AUTOTUNE_PERCENTILE_SQRT_OVER_NME)
    return fail(h, SC_ERR_INVALID, "Unsupported value of AutoTuneProxy");
  {
    bool has_threshold = false;
    for (int i = 0; i < cfg->n_ops; ++i) has_threshold |= cfg->ops[i] == SC_OP_ROW_WISE_THRESHOLD;
    if (!has_threshold)
      return fail(h, SC_ERR_INVALID,
                  "AutoTune is only effective when the refinement sequence"
                  "contains RowWiseThreshold");
  }
  SC_HIP(h, hipSetDevice(h->device));
  bool device_source = false;
  std::vector<int> ns;
  int d = 0;
  SC_TRY(validate_batch_arrays(h, xs, count, &ns, &d, &device_source, labels));
  SC_TRY(sc_clear_constraint(h));  // the handle's own resident constraint takes no part
  h->last_routes.assign(count, SC_BATCH_ROUTE_SINGLE);
  if (count == 0) return SC_OK;
  if (device_source) SC_HIP(h, hipStreamSynchronize(h->stream));  // (as sc_predict_batch_arrays)
  const EigRequest rq = make_eig_request(cfg);
  // no band stays resident in any arena, and none is still on its way up, however the batch ends
  struct Cleanup {
    sc_handle h;
    int rc = SC_OK;
    ~Cleanup() {
      for (sc_handle sub : h->gshort) {
        if (rc != SC_OK) (void)hipStreamSynchronize(sub->stream);
        (void)sc_clear_constraint(sub);
      }
      for (sc_handle lane : h->glanes) (void)sc_clear_constraint(lane);
      (void)sc_clear_constraint(h);
    }
  } cleanup{h};
  // ---- partition
  // (which sequences the sweep groups: the configuration alone decides)
  const bool swept = swept_sequence(cfg, nullptr) && cfg->kmeans_metric == kKmeansCosine &&
                     !(cfg->constraint_name != SC_CONSTRAINT_NONE && !cfg->constraint_before_refinement);
  std::vector<int> shorts, mids, single;
  for (int i = 0; i < count; ++i) {
    if (swept && ns[i] > 0 && ns[i] <= kDenseMax) shorts.push_back(i);
    else if (swept && sym_group_eligible(ns[i], rq)) mids.push_back(i);
    else single.push_back(i);
  }
  {  // do the arenas fit?  the short route: 2 x kShortWidth arenas of n = kDenseMax; a lane: a
     // level's members (two matrices each) at its largest utterance.  Otherwise: route 0.
    size_t free_b = 0, total_b = 0;
    SC_HIP(h, hipMemGetInfo(&free_b, &total_b));
    int largest = 0;
    for (int i : mids) largest = std::max(largest, ns[i]);
    const size_t arena = (size_t)80 << 20;  // (the allocator's granule per small arena)
    size_t need = shorts.empty() ? 0 : 2 * (size_t)kShortWidth * arena;
    need += (size_t)kGroupLanes * kGroupMax * (2 * (size_t)largest * matrix_ld(std::max(largest, 1)) *
                                               sizeof(double) + (size_t)largest * 8192);
    if ((double)need > 0.85 * (double)free_b) {
      single.insert(single.end(), shorts.begin(), shorts.end());
      single.insert(single.end(), mids.begin(), mids.end());
      shorts.clear();
      mids.clear();
      std::sort(single.begin(), single.end());
    }
  }
  // ---- 128 < n < 4096: dealt longest-first to the lanes, each its own handle, stream and thread
  std::stable_sort(mids.begin(), mids.end(), [&](int a, int b) { return ns[a] > ns[b]; });
  const int lanes = std::max(1, std::min(kGroupLanes, (int)mids.size()));
  std::vector<int> lane_list[kGroupLanes];
  deal_least_loaded(mids, [&](int i) { return unit_cost(ns[i]); }, lanes, lane_list);
  sc_handle leads[kGroupLanes] = {h};
  // (h->groutes is null here: the lanes report through `routes` below)
  cleanup.rc = ensure_lanes(h, lanes, "AutoTune batch", leads);
  if (cleanup.rc != SC_OK) return cleanup.rc;
  int32_t* routes = h->last_routes.data();
  auto search_one = [&](sc_handle on, int i) {  // utterance i as a single search on handle `on`
    return autotune_one(on, xs[i], bands ? bands[i] : nullptr, cfg, at, labels[i],
                        diags ? diags + i : nullptr, best_p ? best_p + i : nullptr,
                        last_p ? last_p + i : nullptr);
  };
  auto run_lane = [&](int l) -> int {
    sc_handle lead = leads[l];
    if (hipSetDevice(lead->device) != hipSuccess) return SC_ERR_HIP;
    for (int i : lane_list[l]) {
      const int rc = search_one(lead, i);
      if (rc != SC_OK) return rc;
      routes[i] = SC_BATCH_ROUTE_GROUP_LANCZOS;
    }
    return SC_OK;
  };
  int lane_rc[kGroupLanes] = {SC_OK, SC_OK, SC_OK};
  std::vector<std::thread> workers;
  for (int l = 1; l < lanes; ++l) workers.emplace_back([&, l] { lane_rc[l] = run_lane(l); });
  // ---- n <= 128 on the caller's thread: waves of kShortWidth utterances, largest first
  int rc = SC_OK;
  std::stable_sort(shorts.begin(), shorts.end(), [&](int a, int b) { return ns[a] > ns[b]; });
  if (!shorts.empty()) rc = ensure_seed_table(h);
  h->sweep_slot.clear();  // (the pair arenas are the sweep's member arenas)
  h->groutes = routes;
  for (size_t at0 = 0; at0 < shorts.size() && rc == SC_OK; at0 += kShortWidth)
    rc = autotune_short_wave(h, xs, bands, ns.data(), d, cfg, at, rq, shorts.data() + at0,
                             (int)std::min<size_t>(kShortWidth, shorts.size() - at0), labels, diags,
                             best_p, last_p, &single);
  h->groutes = nullptr;
  if (rc == SC_OK && !mids.empty()) rc = lane_rc[0] = run_lane(0);
  for (std::thread& t : workers) t.join();
  for (int l = 1; l < lanes && rc == SC_OK; ++l)
    if (lane_rc[l] != SC_OK) rc = fail(h, lane_rc[l], leads[l]->err);
  // ---- n >= 4096, sequences the sweep does not group, members that left their route
  std::sort(single.begin(), single.end());
  for (size_t q = 0; q < single.size() && rc == SC_OK; ++q) {
    rc = search_one(h, single[q]);
    routes[single[q]] = SC_BATCH_ROUTE_SINGLE;
  }
  return cleanup.rc = rc;
}
