// AutoTune: one search level as a group (reference autotune.py:98-111).  The values of a level
// differ in nothing but the row threshold: what they share runs once, the per-value front is
// grouped launches over member arenas (one per value, the lead's gslots), the solve ONE lockstep
// block Lanczos (eig_driver.hip: sym_topk_group) -- or, at n <= kDenseMax, one front launch and
// one dense Jacobi launch for up to kShortWidth (matrix, p) pairs.  The AutoTune batch
// (batch_autotune.hip) runs the pairs of many utterances through the same pieces.
#include "batch_internal.h"

// Two sequences are swept as groups: the ICASSP2018 one, and [RowWiseThreshold, Symmetrize]
// alone -- the Turn-to-Diarize refinement (reference configs.py:49-59: Percentile cut,
// binarisation, preserved diagonal, Average), whose values are the thresholded affinity
// itself: no blur to share, no Diffuse, the lockstep solver works on the symmetrised matrix.
bool swept_sequence(const sc_config* cfg, SweepPlan* plan) {
  const bool icassp = grouped_front_covers(cfg);
  const bool thr_sym_only = cfg->n_ops == 2 && cfg->ops[0] == SC_OP_ROW_WISE_THRESHOLD &&
                            cfg->ops[1] == SC_OP_SYMMETRIZE;
  if (plan) {
    plan->icassp = icassp;
    plan->thr_sym_only = thr_sym_only;
  }
  return icassp || thr_sym_only;
}

SweepPlan sweep_plan(sc_handle h, const sc_config* cfg, int count, const EigRequest& rq) {
  const int n = h->n;
  SweepPlan plan;
  const bool swept = swept_sequence(cfg, &plan);
  plan.grouped = count > 1 && swept && h->affinity_symmetric &&
                 !constraint_active(h, cfg, false) &&
                 (!plan.icassp || blur_group_supported(n, cfg->blur_radius)) &&
                 sym_group_eligible(n, rq, true) && !sw::sweep_one_by_one();
  // Matrix-free Diffuse (free_api.hip): a member then holds the thresholded matrix, its digits
  // and the fp32 tiles of their product instead of S, and the lockstep solver applies A twice.
  // The cut vector bounds max|a| when the affinity is non-negative by construction.
  plan.free_route = plan.icassp && free_diffuse_wanted(h, cfg, n, rq);
  plan.amax_from_cut = plan.free_route && h->affinity_from_embeddings &&
                       !h->constraint_applied && cfg->soft_multiplier >= 0.0 &&
                       cfg->soft_multiplier <= 1.0;
  // A level of a short utterance ends in the one-workgroup Jacobi solve per value: evaluated one
  // by one that is count launches on ONE CU each.  The same two sequences, under the same
  // conditions, go through the short front and dense_topk_group instead.
  plan.short_level = !plan.grouped && count > 1 && n <= kDenseMax && swept &&
                     h->affinity_symmetric && !constraint_active(h, cfg, false) &&
                     !plan.free_route && !sw::sweep_one_by_one();
  return plan;
}

// The part of the ICASSP2018 front every value of a level shares: CropDiagonal's value and the
// blurred matrix (+ per-strip row maxima) of the resident affinity, on the handle's stream.
// `crop` (may be null): where the value vector the blur read lies; `crop_source`: as FrontResult's.
int sweep_shared_blur(sc_handle h, const sc_config* cfg, const double** crop_out,
                      int* crop_source) {
  const int n = h->n, ld = h->ldn;
  hipStream_t s = h->stream;
  // ---- shared by every value: CropDiagonal's value and the blurred matrix (+ row maxima)
  const double* crop = ptr<double>(h->cropval);
  if (crop_source) *crop_source = 1;
  if (!h->have_cropval) {
    launch_crop_value(s, ptr<double>(h->A0), n, ld, ptr<double>(h->dvec));
    crop = ptr<double>(h->dvec);
    if (crop_source) *crop_source = 2;
  }
  if (crop_out) *crop_out = crop;
  SC_TRY(upload_blur_weights(h, cfg));
  if (!launch_gaussian_blur_fused(s, ptr<double>(h->A0), ptr<double>(h->B1), n, ld,
                                  cfg->blur_radius, ptr<double>(h->blurw), crop,
                                  ptr<double>(h->rmpart), &h->last_blur))
    return fail(h, SC_ERR_HIP, "fused blur not taken");
  SC_TRY(check_last(h, "sweep blur launch"));
  return SC_OK;
}

// The members of one round (value ps[z] in member arena z): arenas sized, launch descriptors
// filled.  `slot0`: the first member arena to use; `owner`: the handle whose arenas they are
// (default: h's own -- an AutoTune batch keeps the pairs of many utterances in the lead's).
// *out_of_memory (with SC_OK): an arena's buffers did not fit -- the sweep runs the rest one by
// one.  Any other failure, creating an arena included, is returned.
int sweep_round_members(sc_handle h, const sc_config* cfg, const SweepPlan& plan,
                        const EigRequest& rq, const double* ps, int cnt, FrontItem* fi,
                        GemmGroupItem* dif, GroupEigMember* em, bool* out_of_memory,
                        int slot0, sc_handle owner) {
  *out_of_memory = false;
  const int n = h->n, ld = h->ldn;
  const bool icassp = plan.icassp, free_route = plan.free_route;
  for (int z = 0; z < cnt; ++z) {
    sc_handle hz = nullptr;
    SC_TRY(group_slot(owner ? owner : h, slot0 + z, &hz));
    int rc = ensure_matrices(hz, n, 0, false);
    if (rc == SC_OK) rc = ensure_eig(hz, n);
    if (rc == SC_OK) rc = ensure_tilemap(hz, n);
    if (rc == SC_OK && free_route) rc = ensure_free(hz, n);
    if (rc == SC_ERR_OOM) {  // the caller's estimate was optimistic: the rest one by one
      *out_of_memory = true;
      return SC_OK;
    }
    if (rc != SC_OK) return fail(h, rc, hz->err);
    hz->n = n;
    hz->ldn = ld;
    hz->n_vec = 0;
    // the arena holds what the value's refinement leaves; what it reads is the lead's:
    FrontItem& f = fi[z];
    f = front_item(hz, kFrontRefined);
    // the matrix every value thresholds: the shared blurred one, or the affinity itself
    f.B1 = icassp ? ptr<double>(h->B1) : ptr<double>(h->A0);  // read only
    f.rmpart = ptr<double>(h->rmpart);  // (of the shared blur)
    f.blur_cols = blur_tile_columns(n, cfg->blur_radius);
    // (the lead's rows were normalised; an affinity that was set has no such word)
    f.symflag = h->affinity_from_embeddings ? ptr<int>(h->symflag) : nullptr;
    f.p_own = ps[z];
    dif[z] = diffuse_item(hz, true);
    em[z] = GroupEigMember();
    em[z].h = hz;
    em[z].S = (free_route || !icassp) ? ptr<double>(hz->B2) : ptr<double>(hz->B1);
    em[z].ld = ld;
    em[z].n = n;
    em[z].rq = rq;
    em[z].free_op = free_route;
  }
  return SC_OK;
}

// The front of one round, for its `cnt` members: cuts (p_own per member), the grouped threshold +
// symmetrise pass with or without digits, Diffuse or its statistics, the scaling vectors -- all on
// the handle's stream.  sc_eig_ncluster_sweep runs the lockstep solver behind it; sc_stage_front
// copies out what it left.
// `taken` (may be null): per member, which kernel made its cut, whether the threshold pass wrote
// its digits and whether the fp64 product formed its S (FrontResult's fields), set where each
// launch happens.
int sweep_round_front(sc_handle h, const sc_config* cfg, const SweepPlan& plan, const double* ps,
                      int cnt, FrontItem* fi, GemmGroupItem* dif, GroupEigMember* em,
                      FrontResult* taken) {
  const int n = h->n, ld = h->ldn;
  hipStream_t s = h->stream;
  const bool icassp = plan.icassp, free_route = plan.free_route;
  const bool amax_from_cut = plan.amax_from_cut;
  {  // (the init kernel must not clear the shared symflag word)
    FrontItem init[kGroupMax];
    memcpy(init, fi, sizeof(init));
    for (int z = 0; z < cnt; ++z) init[z].symflag = nullptr;
    launch_front_begin_group(s, init, cnt, false);
  }
  const bool own_cuts = !icassp;  // (RowMax cuts of the ICASSP front come from the blur's partials)
  if (own_cuts) {
    if (cfg->threshold_type == SC_THRESHOLD_PERCENTILE) {
      launch_cut_percentile_group(s, fi, cnt, cfg->preserve_diagonal);  // (p_own per member)
      for (int z = 0; taken && z < cnt; ++z) taken[z].cut_kernel = 3;
    } else {
      for (int z = 0; z < cnt; ++z)
        launch_cut_from_rows(s, fi[z].B1, n, ld, ps[z], fi[z].cut,
                             cfg->preserve_diagonal);
      for (int z = 0; taken && z < cnt; ++z) taken[z].cut_kernel = 2;
    }
  }
  // (round 6: with max|a| known from the cuts the threshold pass writes the members' digits
  //  itself -- free_group_prepare / free_group_digits, free_api.hip; amax_from_cut implies
  //  icassp and free_route)
  FreeItem fitems[kGroupMax];
  if (amax_from_cut) {
    sc_handle fh0[kGroupMax];
    const double* mats[kGroupMax];
    const double* cuts[kGroupMax];
    int nn[kGroupMax], ll[kGroupMax];
    for (int z = 0; z < cnt; ++z) {
      fh0[z] = em[z].h;
      mats[z] = em[z].S;
      cuts[z] = ptr<double>(em[z].h->cut);
      nn[z] = n;
      ll[z] = ld;
    }
    if (!own_cuts) launch_cut_from_partials_group(s, fi, cnt, cfg->p_percentile);
    TsDigits digits[kGroupMax];
    SC_TRY(free_group_prepare(fh0, mats, cuts, ps, cnt, ll, nn, s,
                              (cfg->binarize || cfg->preserve_diagonal) ? 1.0 : 0.0, fitems,
                              digits));
    launch_threshold_symmetrize_group(s, fi, cnt, cfg->p_percentile, cfg->soft_multiplier,
                                      cfg->binarize, cfg->symmetrize_type,
                                      cfg->preserve_diagonal, true, digits);
    for (int z = 0; taken && z < cnt; ++z) {
      if (!own_cuts) taken[z].cut_kernel = 1;  // launch_cut_from_partials_group above
      taken[z].digits_fused = digits[z].Q != nullptr;
    }
  } else {
    launch_threshold_symmetrize_group(s, fi, cnt, cfg->p_percentile, cfg->soft_multiplier,
                                      cfg->binarize, cfg->symmetrize_type,
                                      cfg->preserve_diagonal, own_cuts);
    // (cut_ready false: the launcher takes the cuts from the blur's partials itself)
    for (int z = 0; taken && !own_cuts && z < cnt; ++z) taken[z].cut_kernel = 1;
  }
  if (!icassp) {
    // no Diffuse: the row sums of the symmetrised matrix are the degrees
    launch_row_stats_group(s, fi, cnt);
  } else if (free_route) {
    // rowmax / rowsum of every member's S = A A^T without forming it: digits per member,
    // ONE launch for the digit products of all members, candidates + exact recheck per member
    const signed char* qs[kGroupMax];
    float* ts[kGroupMax];
    unsigned* ms[kGroupMax];
    sc_handle fh[kGroupMax];
    for (int z = 0; z < cnt; ++z) fh[z] = em[z].h;
    if (amax_from_cut) {
      SC_TRY(free_group_digits(fh, fitems, cnt, s));
    } else {
      for (int z = 0; z < cnt; ++z) SC_TRY(free_stats_begin(em[z].h, s, em[z].S, ld, n, false));
    }
    for (int z = 0; z < cnt; ++z) {
      sc_handle hz = em[z].h;
      qs[z] = ptr<signed char>(hz->fq);
      ts[z] = ptr<float>(hz->ft32);
      ms[z] = ptr<unsigned>(hz->fwords);
    }
    {
      int nn[kGroupMax];
      const int2* tms[kGroupMax];
      const int* pls[kGroupMax];
      for (int z = 0; z < cnt; ++z) {
        nn[z] = n;
        tms[z] = em[0].h->tilemap_cur;
        pls[z] = amax_from_cut ? fitems[z].plan : nullptr;
      }
      launch_gemm_i8_sym_group(s, qs, ts, ms, cnt, nn, tms, pls);
    }
    if (amax_from_cut) {
      SC_TRY(free_group_end(fh, fitems, cnt, s));
    } else {
      for (int z = 0; z < cnt; ++z) SC_TRY(free_stats_end(em[z].h, s, em[z].S, ld, n, false));
    }
  } else {
    launch_gemm_nt_group(s, dif, cnt, kEpiNone, 1);
    for (int z = 0; taken && z < cnt; ++z) taken[z].diffuse_explicit = dif[z].n > 0;
  }
  launch_scaling_vectors_group(s, fi, cnt, cfg->laplacian_type, icassp ? 1 : 0);
  SC_TRY(check_last(h, "sweep launch"));
  return SC_OK;
}

// ---- a level of a short utterance (n <= kDenseMax, plan.short_level)
// What every value of the level shares, with the single call's kernels: nothing for
// [RowWiseThreshold, Symmetrize]; CropDiagonal + GaussianBlur for the ICASSP2018 sequence -- the
// two unfused kernels below n = 128 (crop into B1, blur into B2), value vector + fused blur at 128.
int sweep_short_shared(sc_handle h, const sc_config* cfg, const SweepPlan& plan, ShortShared* sh) {
  const int n = h->n, ld = h->ldn;
  *sh = ShortShared();
  sh->src = ptr<double>(h->A0);
  if (!plan.icassp) return SC_OK;
  if (n >= 128) {  // (eig_ncluster_impl's blur_fast; the radius is 4 or 8: grouped_front_covers)
    SC_TRY(sweep_shared_blur(h, cfg, &sh->crop, &sh->crop_source));
    sh->src = ptr<double>(h->B1);
    return SC_OK;
  }
  SC_TRY(run_refine_op(h, SC_OP_CROP_DIAGONAL, cfg, ptr<double>(h->A0), ptr<double>(h->B1), n, ld));
  SC_TRY(run_refine_op(h, SC_OP_GAUSSIAN_BLUR, cfg, ptr<double>(h->B1), ptr<double>(h->B2), n, ld));
  sh->src = ptr<double>(h->B2);
  return SC_OK;
}

// The per-value front of up to kShortWidth (matrix, p) pairs whose member arenas are set up (fi,
// dif: pair z thresholds srcs[z] at ps[z]) on the lead's stream: ONE k_short_sweep_front launch;
// for the ICASSP2018 sequence the Diffuse product and the scaling vectors follow through the
// grouped launchers, kGroupMax pairs per launch.  The pairs may belong to different utterances.
int short_pairs_launch(sc_handle h, const sc_config* cfg, const SweepPlan& plan,
                       const double* const* srcs, const double* ps, int cnt, const FrontItem* fi,
                       const GemmGroupItem* dif) {
  hipStream_t s = h->stream;
  const size_t bytes = (size_t)kShortWidth * sizeof(ShortFrontItem);
  SC_TRY(grow(h, h->gsftab, bytes));
  if (!h->h_gsftab) {
    SC_HIP(h, hipHostMalloc(reinterpret_cast<void**>(&h->h_gsftab), bytes));
    SC_HIP(h, hipEventCreateWithFlags(&h->gsftab_ev, hipEventDisableTiming));
  } else {
    // the pinned table is rewritten: the copy of the launch before must have read it (it has,
    // wherever a Jacobi launch and its synchronisation followed: no stall then)
    SC_HIP(h, hipEventSynchronize(h->gsftab_ev));
  }
  for (int z = 0; z < cnt; ++z) {
    ShortFrontItem& it = h->h_gsftab[z];
    it = ShortFrontItem();
    it.src = srcs[z];
    it.n = fi[z].n;
    it.ld = fi[z].ldn;
    it.p = ps[z];
    it.out = fi[z].B2;
    it.cut = fi[z].cut;
    if (!plan.icassp) {  // no Diffuse: the kernel leaves the statistics and the operator's vectors
      it.rowmax = const_cast<double*>(fi[z].rowmax);
      it.rowsum = const_cast<double*>(fi[z].rowsum);
      it.cvec = fi[z].cvec;
      it.pvec = fi[z].pvec;
      it.tvec = fi[z].tvec;
    }
    it.flags = fi[z].flags;
    it.symflag = fi[z].symflag;
  }
  SC_HIP(h, hipMemcpyAsync(h->gsftab.p, h->h_gsftab, (size_t)cnt * sizeof(ShortFrontItem),
                           hipMemcpyHostToDevice, s));
  SC_HIP(h, hipEventRecord(h->gsftab_ev, s));
  launch_short_sweep_front(s, ptr<ShortFrontItem>(h->gsftab), cnt, cfg->threshold_type,
                           cfg->soft_multiplier, cfg->binarize, cfg->symmetrize_type,
                           cfg->preserve_diagonal, cfg->laplacian_type);
  for (int at = 0; plan.icassp && at < cnt; at += kGroupMax) {
    const int c = std::min(kGroupMax, cnt - at);
    FrontItem init[kGroupMax];  // (the init kernel must not clear the shared symflag word)
    memset(init, 0, sizeof(init));
    for (int z = 0; z < c; ++z) {
      init[z] = fi[at + z];
      init[z].symflag = nullptr;
    }
    launch_front_begin_group(s, init, c, false);
    launch_gemm_nt_group(s, dif + at, c, kEpiNone, 1);
    launch_scaling_vectors_group(s, fi + at, c, cfg->laplacian_type, 1);
  }
  SC_TRY(check_last(h, "short sweep launch"));
  return SC_OK;
}

// ... of one utterance's level: value ps[z] in member arena z.  fi / dif / em: kShortWidth entries
// each.  *out_of_memory as sweep_round_members'.
int sweep_short_front(sc_handle h, const sc_config* cfg, const SweepPlan& plan,
                      const EigRequest& rq, const ShortShared& sh, const double* ps, int cnt,
                      FrontItem* fi, GemmGroupItem* dif, GroupEigMember* em, bool* out_of_memory) {
  *out_of_memory = false;
  for (int at = 0; at < cnt && !*out_of_memory; at += kGroupMax)
    SC_TRY(sweep_round_members(h, cfg, plan, rq, ps + at, std::min(kGroupMax, cnt - at), fi + at,
                               dif + at, em + at, out_of_memory, at));
  if (*out_of_memory) return SC_OK;
  const double* srcs[kShortWidth];
  for (int z = 0; z < cnt; ++z) srcs[z] = sh.src;
  return short_pairs_launch(h, cfg, plan, srcs, ps, cnt, fi, dif);
}

namespace {
// A value outside the group: its own sc_eig_ncluster (which states the error, or finds what the
// group did not)
int sweep_single_value(sc_handle h, const sc_config* cfg, double p, sc_diag* diag) {
  sc_config c = *cfg;
  c.p_percentile = p;
  return sc_eig_ncluster(h, &c, diag);
}

// What sc_eig_ncluster reports for a value the group solved (`path`: the solver that did)
void sweep_value_diag(sc_diag* dg, const GroupEigMember& g, const SweepPlan& plan,
                      const EigRequest& rq, int path) {
  memset(dg, 0, sizeof(*dg));
  dg->n = g.n;
  dg->n_clusters_raw = g.dc.n_clusters_raw;
  dg->max_delta = g.dc.max_delta;
  dg->eig_descending = rq.descend;
  dg->n_eigenvalues = std::min((int)g.w.size(), SC_MAX_EIG);
  for (int i = 0; i < dg->n_eigenvalues; ++i) dg->eigenvalues[i] = g.w[i];
  dg->symmetry_state = plan.icassp ? 2 : 1;
  dg->eig_path = path;
  if (path == SC_EIG_PATH_BLOCK_LANCZOS) {  // (the dense solve has no basis to report)
    dg->eig_matvec_passes = g.passes;
    dg->eig_block = kEigBlock;
    dg->eig_basis = g.basis;
    dg->eig_max_residual = g.dc.max_resid;
  }
  dg->diffuse_path = !plan.icassp ? SC_DIFFUSE_PATH_NONE
                                  : (plan.free_route ? SC_DIFFUSE_PATH_FREE : SC_DIFFUSE_PATH_EXPLICIT);
  if (plan.free_route) {
    dg->free_candidates = g.h->h_free[65];
    dg->free_tiles_run = g.h->h_free[67];
  }
}

// sc_eig_ncluster_sweep for plan.short_level: the level's values in launches of up to kShortWidth
// pairs, each ONE front launch and ONE Jacobi launch (dense_topk_group: a workgroup per pair, the
// kernel body of the value's own sc_eig_ncluster).  Every solved value's eigenvectors stay in its
// member arena (sc_sweep_adopt).  *handled false: nothing was evaluated, the caller goes one by
// one.
int sweep_short_level(sc_handle h, const sc_config* cfg, const SweepPlan& plan,
                      const EigRequest& rq, const double* p_values, int count, sc_diag* diags,
                      bool* handled) {
  const int n = h->n;
  *handled = false;
  ShortShared sh;
  SC_TRY(sweep_short_shared(h, cfg, plan, &sh));
  std::vector<FrontItem> fi(kShortWidth);
  std::vector<GemmGroupItem> dif(kShortWidth);
  std::vector<GroupEigMember> em(kShortWidth);
  h->sweep_slot.assign(count, -1);
  h->sweep_n = n;
  h->sweep_p.assign(p_values, p_values + count);
  h->sweep_cfg = *cfg;
  std::vector<int> later;  // values whose request the dense solve could not satisfy
  for (int base = 0; base < count; base += kShortWidth) {
    const int cnt = std::min(kShortWidth, count - base);
    memset(fi.data(), 0, fi.size() * sizeof(FrontItem));
    bool out_of_memory = false;
    SC_TRY(sweep_short_front(h, cfg, plan, rq, sh, p_values + base, cnt, fi.data(), dif.data(),
                             em.data(), &out_of_memory));
    if (out_of_memory) {
      (void)hipGetLastError();
      if (base == 0) {
        h->sweep_slot.clear();
        return SC_OK;
      }
      for (int i = base; i < count; ++i) later.push_back(i);
      break;
    }
    SC_TRY(dense_topk_group(h, em.data(), cnt));
    for (int& slot : h->sweep_slot)
      if (slot >= 0 && slot < cnt) slot = -1;  // an earlier launch's member: arena reused
    for (int z = 0; z < cnt; ++z) {
      if (em[z].status != 0) {
        later.push_back(base + z);
        continue;
      }
      h->sweep_slot[base + z] = z;
      sweep_value_diag(diags + base + z, em[z], plan, rq, SC_EIG_PATH_DENSE_JACOBI);
    }
  }
  *handled = true;
  for (int i : later) SC_TRY(sweep_single_value(h, cfg, p_values[i], diags + i));
  h->n_vec = 0;  // nothing of any member is resident in this handle
  h->sweep_diags.assign(diags, diags + count);
  return SC_OK;
}
}  // namespace

// ------------------------------------------------------------------------------
// AutoTune: one search level as a group (reference autotune.py:98-111)
// ------------------------------------------------------------------------------
// sc_eig_ncluster for `count` values of p_percentile on the resident affinity.  The values of
// a level differ in nothing but the row threshold: CropDiagonal + GaussianBlur run once, then
// the members (one per value, up to kGroupMax per round) go through threshold + symmetrise,
// the Diffuse GEMM (all members' tiles in one launch) and the scaling vectors as grouped
// launches and through ONE lockstep block Lanczos (sym_topk_group, eigenvalues + eigengap
// decision only).  diags[i] is what sc_eig_ncluster would report for p_values[i]; no
// eigenvectors are left resident (evaluate the winner with sc_eig_ncluster).  At n <= kDenseMax
// the values are (matrix, p) pairs of one front launch and one dense Jacobi launch
// (sweep_short_level).  Configurations the grouped stages do not cover are evaluated one by one.
extern "C" int sc_eig_ncluster_sweep(sc_handle h, const sc_config* cfg, const double* p_values,
                                     int count, sc_diag* diags) {
  if (!h) return SC_ERR_INVALID;
  if (!p_values || !diags || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  SC_TRY(validate_config(h, cfg));
  if (!h->have_affinity) return fail(h, SC_ERR_INVALID, "no affinity resident");
  SC_HIP(h, hipSetDevice(h->device));
  const int n = h->n, ld = h->ldn;
  const EigRequest rq = make_eig_request(cfg);
  // whatever an earlier sweep left in the member arenas is no longer adoptable (a sweep that
  // takes the one-by-one route below leaves no eigenvectors there at all)
  h->sweep_slot.clear();
  auto one_by_one = [&](int i) { return sweep_single_value(h, cfg, p_values[i], diags + i); };
  const SweepPlan plan = sweep_plan(h, cfg, count, rq);
  const bool icassp = plan.icassp, free_route = plan.free_route;
  if (plan.short_level) {
    bool handled = false;
    SC_TRY(sweep_short_level(h, cfg, plan, rq, p_values, count, diags, &handled));
    if (handled) return SC_OK;
  }
  if (!plan.grouped) {
    for (int i = 0; i < count; ++i) SC_TRY(one_by_one(i));
    return SC_OK;
  }
  hipStream_t s = h->stream;
  if (icassp) SC_TRY(sweep_shared_blur(h, cfg));
  memset(h->gconv_hist, 0, sizeof(h->gconv_hist));
  h->gconv_seen = 0;
  std::vector<int> later;  // values whose solve left the common path
  h->sweep_slot.assign(count, -1);  // which member arena holds value i's eigenvectors
  h->sweep_n = n;
  h->sweep_p.assign(p_values, p_values + count);
  h->sweep_cfg = *cfg;
  // A member arena of a sweep holds the thresholded matrix (B2), its Diffuse product (B1),
  // the n-vectors and the eigensolver workspace -- no affinity copy, no k-means workspace.
  // The group is as wide as free memory allows (16 members of n = 16384 are 69 GB); whatever
  // does not fit is evaluated one value at a time on this handle, like before the grouping.
  const size_t member_bytes = 2 * (size_t)n * ld * sizeof(double) + (size_t)n * 8192 +
                              (free_route ? free_q_bytes(n) + free_t32_bytes(n) : 0);
  int width = 0;
  {
    size_t free_b = 0, total_b = 0;
    SC_HIP(h, hipMemGetInfo(&free_b, &total_b));
    size_t budget = (size_t)(0.85 * (double)free_b);
    for (; width < std::min(kGroupMax, count); ++width) {
      const bool ready = width < (int)h->gslots.size() &&
                         h->gslots[width]->B1.bytes >= (size_t)n * ld * sizeof(double) &&
                         h->gslots[width]->B2.bytes >= (size_t)n * ld * sizeof(double) &&
                         h->gslots[width]->Q.bytes > 0;
      if (ready) continue;
      if (budget < member_bytes) break;
      budget -= member_bytes;
    }
  }
  if (width < 2) {
    for (int i = 0; i < count; ++i) SC_TRY(one_by_one(i));
    return SC_OK;
  }
  bool out_of_memory = false;
  for (int base = 0; base < count && !out_of_memory; base += width) {
    const int cnt = std::min(width, count - base);
    FrontItem fi[kGroupMax];
    GemmGroupItem dif[kGroupMax];
    GroupEigMember em[kGroupMax];
    memset(fi, 0, sizeof(fi));
    SC_TRY(sweep_round_members(h, cfg, plan, rq, p_values + base, cnt, fi, dif, em,
                               &out_of_memory));
    if (out_of_memory) {
      (void)hipGetLastError();
      for (int i = base; i < count; ++i) later.push_back(i);
      break;
    }
    SC_TRY(sweep_round_front(h, cfg, plan, p_values + base, cnt, fi, dif, em));
    // (with the Ritz vectors: the level's winner is then adopted, not evaluated again --
    //  one upload and one launch for the whole group against a Diffuse + a solve)
    SC_TRY(sym_topk_group(h, em, cnt, true));
    if (free_route) {
      // a value with rows the candidate search could not prune (their exact evaluation needs
      // the host in the loop) goes through the single-call route, like any value that left
      // the lockstep solver: the overflow words arrived with the solver's synchronisations
      SC_HIP(h, hipStreamSynchronize(s));
      for (int z = 0; z < cnt; ++z)
        if (em[z].status == 0 && em[z].h->h_free[0] != 0) em[z].status = 1;
    }
    for (int& slot : h->sweep_slot)
      if (slot >= 0 && slot < cnt) slot = -1;  // an earlier round's member: arena reused
    for (int z = 0; z < cnt; ++z) {
      if (em[z].status != 0) {
        later.push_back(base + z);  // (after the rounds: it overwrites the shared blur)
        continue;
      }
      h->sweep_slot[base + z] = z;
      sweep_value_diag(diags + base + z, em[z], plan, rq, SC_EIG_PATH_BLOCK_LANCZOS);
    }
  }
  SC_HIP(h, hipStreamSynchronize(s));
  // member arenas that hold a large share of the device do not outlive the sweep, and none does
  // after one of them did not fit: no value is adoptable then
  if (release_large_arenas(&h, 1, out_of_memory)) h->sweep_slot.assign(count, -1);
  for (int i : later) SC_TRY(one_by_one(i));  // the single-call solver
  h->n_vec = 0;  // nothing of any member is resident in this handle
  h->sweep_diags.assign(diags, diags + count);
  return SC_OK;
}

// The eigenvectors of value `index` of the last sc_eig_ncluster_sweep become the handle's
// resident eigenvectors (what sc_eig_ncluster with that p_percentile would leave): a copy
// of n x cols doubles out of the member arena instead of a second refinement + Diffuse +
// eigen solve for the AutoTune winner (reference spectral_clusterer.py:274-292 keeps the
// winner's eigenvectors from the search).  `cfg`: the sweep's configuration with p_percentile =
// that value (checked).  SC_ERR_UNSUPPORTED when that value's solve left the grouped path, its
// arena has been reused or the configuration differs: evaluate it with sc_eig_ncluster then.
extern "C" int sc_sweep_adopt(sc_handle h, const sc_config* cfg, int index, sc_diag* diag) {
  if (!h || !cfg) return SC_ERR_INVALID;
  {  // the same configuration as the sweep's, at that value's p_percentile
    sc_config want = h->sweep_cfg;
    if (index >= 0 && index < (int)h->sweep_p.size()) want.p_percentile = h->sweep_p[index];
    if (h->sweep_slot.empty() || memcmp(&want, cfg, sizeof(sc_config)) != 0)
      return fail(h, SC_ERR_UNSUPPORTED, "the last sweep was not run with this configuration");
  }
  if (index < 0 || index >= (int)h->sweep_slot.size() || h->sweep_slot[index] < 0 ||
      h->sweep_slot[index] >= (int)h->gslots.size() || h->sweep_n != h->n ||
      index >= (int)h->sweep_diags.size())
    return fail(h, SC_ERR_UNSUPPORTED, "no eigenvectors of that sweep value are resident");
  SC_HIP(h, hipSetDevice(h->device));
  sc_handle hz = h->gslots[h->sweep_slot[index]];
  const int n = h->n, cols = hz->n_vec;
  if (cols < 1 || hz->n != n)
    return fail(h, SC_ERR_UNSUPPORTED, "no eigenvectors of that sweep value are resident");
  SC_TRY(ensure_eig(h, n));
  SC_HIP(h, hipMemcpyAsync(h->E.p, hz->E.p, (size_t)round_up(n, 16) * cols * sizeof(double),
                           hipMemcpyDeviceToDevice, h->stream));
  h->n_vec = cols;
  h->last_w = hz->last_w;
  if (diag) *diag = h->sweep_diags[index];
  return SC_OK;
}
