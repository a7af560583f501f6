// sc_stage_front: what the fused refinement front leaves behind (tests).  One front of each route
// that has one -- a single call's, the grouped batch's (batch_group.hip: enqueue_front_grouped), a
// round of sc_eig_ncluster_sweep and a launch of its short level (batch_sweep.hip), a wave of the
// short route (enqueue_front_short_wave) -- is enqueued exactly as its route enqueues it, drained,
// and what it wrote is copied out together with the branches it took.
#include "batch_internal.h"

namespace {
// where one member's front left things, and which branches it took
struct FrontWhere {
  sc_handle h = nullptr;  // arena of the n-vectors (rowmax .. tvec, cut) and the overflow record
  int n = 0, ld = 0;
  const double* a0 = nullptr;
  const double* cropval = nullptr;
  const double* cut = nullptr;
  const double* a = nullptr;
  const double* s = nullptr;
  int diffuse_path = SC_DIFFUSE_PATH_NONE;
  bool symmetric = true, folded_rownorm = false, free_op = false, digits_fused = false;
  BlurLaunch blur;
  int crop_source = 0, cut_kernel = 0;
};
// ... for a front whose member arena `hz` holds all of it: the affinity, CropDiagonal's vector,
// A in B2 and -- where the fp64 product formed it -- S in B1; `fr` says which branches it took,
// `lead` made the blur launch.  A route that keeps something elsewhere says so behind the call.
FrontWhere front_where(sc_handle lead, sc_handle hz, int n, const FrontResult& fr) {
  FrontWhere w;
  w.h = hz;
  w.n = n;
  w.ld = hz->ldn;
  w.a0 = ptr<double>(hz->A0);
  w.cropval = ptr<double>(hz->cropval);
  w.cut = fr.cut_kernel != 0 ? ptr<double>(hz->cut) : nullptr;
  w.a = ptr<double>(hz->B2);
  w.s = fr.diffuse_explicit ? ptr<double>(hz->B1) : nullptr;
  w.diffuse_path = fr.free_op ? SC_DIFFUSE_PATH_FREE
                              : (fr.diffuse_explicit ? SC_DIFFUSE_PATH_EXPLICIT
                                                     : SC_DIFFUSE_PATH_NONE);
  w.symmetric = fr.symmetric;
  w.folded_rownorm = fr.folded_rownorm;
  w.free_op = fr.free_op;
  w.digits_fused = fr.digits_fused;
  w.blur = lead->last_blur;
  w.crop_source = fr.crop_source;
  w.cut_kernel = fr.cut_kernel;
  return w;
}

// (every stream of the front has been synchronised: plain blocking copies)
int front_copy_out(sc_handle lead, const FrontWhere& w, sc_front_out* out) {
  const int n = w.n;
  int written = 0;
  auto matrix = [&](const double* src, double* dst, int bit) -> int {
    if (!src || !dst) return SC_OK;
    SC_HIP(lead, hipMemcpy2D(dst, (size_t)n * sizeof(double), src, (size_t)w.ld * sizeof(double),
                             (size_t)n * sizeof(double), n, hipMemcpyDeviceToHost));
    written |= 1 << bit;
    return SC_OK;
  };
  auto vec = [&](const void* src, double* dst, int bit) -> int {
    if (!src || !dst) return SC_OK;
    SC_HIP(lead, hipMemcpy(dst, src, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    written |= 1 << bit;
    return SC_OK;
  };
  SC_TRY(matrix(w.a0, out->a0, 0));
  SC_TRY(vec(w.cropval, out->cropval, 1));
  SC_TRY(vec(w.cut, out->cut, 2));
  SC_TRY(matrix(w.a, out->a, 3));
  SC_TRY(matrix(w.s, out->s, 4));
  SC_TRY(vec(w.h->rowmax.p, out->rowmax, 5));
  SC_TRY(vec(w.h->rowsum.p, out->rowsum, 6));
  SC_TRY(vec(w.h->cvec.p, out->c, 7));
  SC_TRY(vec(w.h->pvec.p, out->p, 8));
  SC_TRY(vec(w.h->tvec.p, out->t, 9));
  int32_t* info = out->info;
  memset(info, 0, sizeof(out->info));
  info[SC_FRONT_INFO_DIFFUSE_PATH] = w.diffuse_path;
  info[SC_FRONT_INFO_SYMMETRIC] = w.symmetric;
  info[SC_FRONT_INFO_FOLDED_ROWNORM] = w.folded_rownorm;
  info[SC_FRONT_INFO_FREE_OP] = w.free_op;
  info[SC_FRONT_INFO_DIGITS_FUSED] = w.digits_fused;
  info[SC_FRONT_INFO_BLUR_KERNEL] = w.blur.kernel;
  info[SC_FRONT_INFO_BLUR_ROWS] = w.blur.rows;
  if (w.free_op) {
    int cand, ovf, forms;
    free_front_info(w.h, &cand, &ovf, &forms);
    info[SC_FRONT_INFO_FREE_CANDIDATES] = cand;
    info[SC_FRONT_INFO_FREE_OVERFLOW_ROWS] = ovf;
    info[SC_FRONT_INFO_FREE_FORMS_S] = forms;
  }
  info[SC_FRONT_INFO_CROP_SOURCE] = w.crop_source;
  info[SC_FRONT_INFO_CUT_KERNEL] = w.cut_kernel;
  info[SC_FRONT_INFO_WRITTEN] = written;
  return SC_OK;
}

// sc_set_embeddings / sc_set_affinity + sc_compute_affinity + the front of sc_eig_ncluster
int stage_front_single(sc_handle h, const sc_config* cfg, int n, int d, const double* x,
                       const double* affinity, sc_front_out* out) {
  if (x) {
    SC_TRY(sc_set_embeddings(h, x, n, d));
    SC_TRY(sc_compute_affinity(h));
  } else {
    SC_TRY(sc_set_affinity(h, affinity, n));
  }
  h->nev = 0;
  sc_diag diag;
  memset(&diag, 0, sizeof(diag));
  FrontResult fr;
  SC_TRY(eig_ncluster_impl(h, cfg, &diag, nullptr, nullptr, false, &fr));
  SC_HIP(h, hipStreamSynchronize(h->stream));
  if (!fr.symmetric)
    return fail(h, SC_ERR_UNSUPPORTED, "sc_stage_front: the refined matrix is not symmetric");
  FrontWhere w = front_where(h, h, n, fr);
  // a single call's sequence is any sequence: the value vector and the matrices are where it says
  w.cropval = fr.crop_source == 1 ? ptr<double>(h->cropval)
                                  : (fr.crop_source == 2 ? ptr<double>(h->dvec) : nullptr);
  // (the explicit product wrote S into the buffer after A's: `scratch` is still A)
  w.a = fr.diffuse_explicit ? fr.scratch : fr.matrix;
  w.s = fr.diffuse_explicit ? fr.matrix : nullptr;
  return front_copy_out(h, w, out);
}

// the members as run_group_lane builds them, then ONE enqueue_front_grouped on bank 0
int stage_front_grouped(sc_handle h, const sc_config* cfg, int count, const int32_t* ns32, int d,
                        const double* const* xs, sc_front_out* outs) {
  const EigRequest rq = make_eig_request(cfg);
  std::vector<int> ns(ns32, ns32 + count), idx(count);
  int largest = 0, smallest = ns[0];
  for (int z = 0; z < count; ++z) {
    idx[z] = z;
    largest = std::max(largest, ns[z]);
    smallest = std::min(smallest, ns[z]);
    // (what predict_batch_core asks of a member of the Lanczos route)
    if (!sym_group_eligible(ns[z], rq))
      return fail(h, SC_ERR_UNSUPPORTED, "sc_stage_front: a member outside the grouped route");
  }
  if (constraint_active(h, cfg, true) || constraint_active(h, cfg, false) ||
      !grouped_front_covers(cfg) || !blur_group_front_supported(smallest, cfg->blur_radius))
    return fail(h, SC_ERR_UNSUPPORTED,
                "sc_stage_front: the grouped front covers the ICASSP2018 sequence (blur radius 4 "
                "or 8, RowMax) on members of n >= 256");
  h->sweep_slot.clear();  // (the member arenas are reused)
  const std::vector<sc_array> arrays = host_f64_arrays(xs, ns.data(), d, count);
  SC_TRY(ensure_bank_stream(h, 0));
  SC_TRY(reserve_bank_arenas(h, cfg, rq, 0, count, largest, d, nullptr));
  SC_TRY(upload_group_blur_weights(h, cfg));
  Member mb[kGroupMax];
  h->last_blur = BlurLaunch();
  const int rc = enqueue_front_grouped(h, arrays.data(), ns.data(), d, cfg, nullptr, idx.data(),
                                       count, 0, mb, 0);
  // (the uploads read the caller's arrays and the statistics write pinned words: drain first)
  SC_HIP(h, hipStreamSynchronize(h->gbank_stream[0]));
  SC_TRY(rc);
  for (int z = 0; z < count; ++z)
    SC_TRY(front_copy_out(h, front_where(h, mb[z].h, ns[z], mb[z].front), outs + z));
  return SC_OK;
}

// the front of one round of sc_eig_ncluster_sweep on the affinity of x
int stage_front_sweep(sc_handle h, const sc_config* cfg, int count, int n, int d, const double* x,
                      const double* p_values, sc_front_out* outs) {
  SC_TRY(sc_set_embeddings(h, x, n, d));
  SC_TRY(sc_compute_affinity(h));
  const EigRequest rq = make_eig_request(cfg);
  const SweepPlan plan = sweep_plan(h, cfg, count, rq);
  if (!plan.grouped)
    return fail(h, SC_ERR_UNSUPPORTED,
                "sc_stage_front: sc_eig_ncluster_sweep would evaluate this level one by one");
  h->last_blur = BlurLaunch();
  const double* crop = nullptr;
  int crop_source = 0;
  if (plan.icassp) SC_TRY(sweep_shared_blur(h, cfg, &crop, &crop_source));
  FrontItem fi[kGroupMax];
  GemmGroupItem dif[kGroupMax];
  GroupEigMember em[kGroupMax];
  FrontResult taken[kGroupMax];
  memset(fi, 0, sizeof(fi));
  bool out_of_memory = false;
  SC_TRY(sweep_round_members(h, cfg, plan, rq, p_values, count, fi, dif, em, &out_of_memory));
  if (out_of_memory)
    return fail(h, SC_ERR_OOM, "sc_stage_front: the round's member arenas do not fit");
  SC_TRY(sweep_round_front(h, cfg, plan, p_values, count, fi, dif, em, taken));
  SC_HIP(h, hipStreamSynchronize(h->stream));
  for (int z = 0; z < count; ++z) {
    FrontResult fr = taken[z];  // (cut_kernel, digits_fused, diffuse_explicit: set at the launches)
    fr.symmetric = true;
    fr.folded_rownorm = plan.icassp;  // (launch_scaling_vectors_group's row_normalized)
    fr.free_op = em[z].free_op;
    fr.crop_source = crop_source;
    FrontWhere w = front_where(h, em[z].h, n, fr);
    w.a0 = ptr<double>(h->A0);  // the affinity and the value vector are the lead's, shared
    w.cropval = crop;
    SC_TRY(front_copy_out(h, w, outs + z));
  }
  return SC_OK;
}

// the front of one launch of a short level (n <= kDenseMax) of sc_eig_ncluster_sweep
int stage_front_short_sweep(sc_handle h, const sc_config* cfg, int count, int n, int d,
                            const double* x, const double* p_values, sc_front_out* outs) {
  SC_TRY(sc_set_embeddings(h, x, n, d));
  SC_TRY(sc_compute_affinity(h));
  const EigRequest rq = make_eig_request(cfg);
  const SweepPlan plan = sweep_plan(h, cfg, count, rq);
  if (!plan.short_level)
    return fail(h, SC_ERR_UNSUPPORTED,
                "sc_stage_front: sc_eig_ncluster_sweep would not run this level as short pairs");
  h->sweep_slot.clear();  // (the member arenas are reused)
  h->last_blur = BlurLaunch();
  ShortShared sh;
  SC_TRY(sweep_short_shared(h, cfg, plan, &sh));
  std::vector<FrontItem> fi(kShortWidth);
  std::vector<GemmGroupItem> dif(kShortWidth);
  std::vector<GroupEigMember> em(kShortWidth);
  memset(fi.data(), 0, fi.size() * sizeof(FrontItem));
  bool out_of_memory = false;
  SC_TRY(sweep_short_front(h, cfg, plan, rq, sh, p_values, count, fi.data(), dif.data(),
                           em.data(), &out_of_memory));
  if (out_of_memory)
    return fail(h, SC_ERR_OOM, "sc_stage_front: the level's member arenas do not fit");
  SC_HIP(h, hipStreamSynchronize(h->stream));
  for (int z = 0; z < count; ++z) {
    FrontResult fr;
    fr.symmetric = true;
    fr.folded_rownorm = fr.diffuse_explicit = plan.icassp;  // (the fp64 product, always)
    fr.crop_source = sh.crop_source;
    fr.cut_kernel = 4;  // launch_short_sweep_front
    FrontWhere w = front_where(h, em[z].h, n, fr);
    w.a0 = ptr<double>(h->A0);  // the affinity and the value vector are the lead's, shared
    w.cropval = sh.crop;
    SC_TRY(front_copy_out(h, w, outs + z));
  }
  return SC_OK;
}

// the front of one wave of the short route of a batch: the members in the order given, arenas and
// table of bank 0 -- enqueue_front_short_wave as run_short_route calls it
int stage_front_short_wave(sc_handle h, const sc_config* cfg, int count, const int32_t* ns32,
                           int d, const double* const* xs, sc_front_out* outs) {
  std::vector<int> ns(ns32, ns32 + count), idx(count);
  for (int z = 0; z < count; ++z) {
    idx[z] = z;
    if (ns[z] > kDenseMax)
      return fail(h, SC_ERR_UNSUPPORTED, "sc_stage_front: a member above 128 rows");
  }
  ShortWaveOps ops;
  if (d > kShortWaveMaxD || constraint_active(h, cfg, true) || constraint_active(h, cfg, false) ||
      !short_wave_covers(cfg, &ops))
    return fail(h, SC_ERR_UNSUPPORTED,
                "sc_stage_front: the short wave front covers d <= 512 and [CropDiagonal] "
                "[GaussianBlur, radius <= 32] RowWiseThreshold Symmetrize [Diffuse] "
                "[RowWiseNormalize] without constraints");
  h->sweep_slot.clear();
  const std::vector<sc_array> arrays = host_f64_arrays(xs, ns.data(), d, count);
  SC_TRY(ensure_bank_stream(h, 0));
  for (int z = 0; z < count; ++z) {
    sc_handle hz = nullptr;
    SC_TRY(group_slot(h, z, &hz, &h->gshort));
    const int rc = sc_reserve(hz, kDenseMax, d);
    if (rc != SC_OK) return fail(h, rc, hz->err);
  }
  if (ops.blur_radius > 0) SC_TRY(upload_group_blur_weights(h, cfg));
  std::vector<Member> mb(count);
  h->gsw_launches = 0;
  const int rc = enqueue_front_short_wave(h, arrays.data(), ns.data(), d, cfg, nullptr, idx.data(),
                                          count, 0, mb.data(), 0, ops);
  SC_HIP(h, hipStreamSynchronize(h->gbank_stream[0]));  // (the uploads read the caller's arrays)
  SC_TRY(rc);
  for (int z = 0; z < count; ++z) {
    FrontWhere w = front_where(h, mb[z].h, ns[z], mb[z].front);
    // (the vector is reported where a single call reports one: its fused crop + blur, which it
    //  takes from n = 128 on at radius 4 or 8 -- below, its CropDiagonal leaves a matrix only)
    const bool single_reports = ops.crop && (ops.blur_radius == 4 || ops.blur_radius == 8) &&
                                ns[z] >= 128;
    if (!single_reports) w.cropval = nullptr;
    if (!single_reports) w.crop_source = 0;
    w.blur = BlurLaunch();  // (the wave kernel blurs in LDS: no blur launch to report)
    SC_TRY(front_copy_out(h, w, outs + z));
    outs[z].info[SC_FRONT_INFO_LAUNCHES] = h->gsw_launches;
  }
  return SC_OK;
}
}  // namespace

extern "C" int sc_stage_front(sc_handle h, int route, const sc_config* cfg, int count,
                              const int32_t* ns, int d, const double* const* xs,
                              const double* affinity, const double* p_values,
                              sc_front_out* outs) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_config(h, cfg));
  if (!ns || !outs || count < 1) return fail(h, SC_ERR_INVALID, "sc_stage_front: NULL argument");
  const bool wide = route == SC_FRONT_ROUTE_SHORT_SWEEP || route == SC_FRONT_ROUTE_SHORT_WAVE;
  if (count > (wide ? kShortWidth : kGroupMax))
    return fail(h, SC_ERR_UNSUPPORTED,
                "sc_stage_front: at most 16 members / values per call (a short level or wave: one "
                "launch of up to 64)");
  SC_HIP(h, hipSetDevice(h->device));
  const int members =
      (route == SC_FRONT_ROUTE_GROUPED || route == SC_FRONT_ROUTE_SHORT_WAVE) ? count : 1;
  for (int z = 0; z < members; ++z)
    if (ns[z] <= 0 || (xs && !xs[z]))
      return fail(h, SC_ERR_INVALID, "sc_stage_front: every member needs rows");
  if (xs ? d <= 0 : (route != SC_FRONT_ROUTE_SINGLE || !affinity))
    return fail(h, SC_ERR_INVALID,
                "sc_stage_front: embeddings (n, d), or an affinity on the single route");
  switch (route) {
    case SC_FRONT_ROUTE_SINGLE:
      if (count != 1) return fail(h, SC_ERR_INVALID, "sc_stage_front: the single route takes one");
      return stage_front_single(h, cfg, ns[0], d, xs ? xs[0] : nullptr, affinity, outs);
    case SC_FRONT_ROUTE_GROUPED:
      return stage_front_grouped(h, cfg, count, ns, d, xs, outs);
    case SC_FRONT_ROUTE_SWEEP:
      if (!p_values) return fail(h, SC_ERR_INVALID, "sc_stage_front: p_values is NULL");
      return stage_front_sweep(h, cfg, count, ns[0], d, xs[0], p_values, outs);
    case SC_FRONT_ROUTE_SHORT_SWEEP:
      if (!p_values) return fail(h, SC_ERR_INVALID, "sc_stage_front: p_values is NULL");
      return stage_front_short_sweep(h, cfg, count, ns[0], d, xs[0], p_values, outs);
    case SC_FRONT_ROUTE_SHORT_WAVE:
      if (!xs) return fail(h, SC_ERR_INVALID, "sc_stage_front: the short wave takes embeddings");
      return stage_front_short_wave(h, cfg, count, ns, d, xs, outs);
  }
  return fail(h, SC_ERR_INVALID, "sc_stage_front: unknown route");
}
