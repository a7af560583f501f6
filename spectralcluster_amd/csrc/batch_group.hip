// Grouped execution of a batch of SHORT utterances (512 independent
// predict() calls, n = 300..3000): groups of up to 16 utterances per launch, dealt to three
// lanes (a lead handle, its streams and a host thread each; sc_predict_batch_grouped below).
//
// A short utterance cannot fill 256 CUs, and after its three GEMM-shaped stages its pipeline
// is ~50 tiny dependent launches (block Lanczos chain, k-means chain) with three host
// synchronisations: 0.45-0.6 ms of latency that does not shrink with n.  Running utterances
// on several streams from several host threads hides that latency (sc_predict_batch_streams);
// this file removes it instead.  Per group:
//   front   upload, affinity GEMM, refinement, Diffuse GEMM, scaling vectors of every member
//           of a group of up to kGroupMax utterances are enqueued back to back, each on the
//           member's own stream (no host synchronisation; one utterance's GEMM tiles cannot
//           fill the chip, several members' do); an event per member hands over to the
//           owner's stream,
//   eigen   ONE lockstep block Lanczos for the group (eig_driver.hip: sym_topk_group): every
//           launch carries one link of every member (blockIdx.y = member, descriptors in the
//           kernel arguments), one synchronisation per Rayleigh-Ritz check for all of them,
//   k-means ONE lockstep chain for the group (kmeans_chain.hip: launch_kmeans_chain_group).
// (When the refinement sequence is the ICASSP2018 one, the front itself is grouped launches
// too -- enqueue_front_grouped: both GEMMs take the tiles of all members in one launch.)
// Each member runs the same kernel bodies with the same arguments as a single call; members
// that leave the common path (rare branches of the eigensolver, k > 32, a non-symmetric
// refinement, n >= 4096) go through the single-call path.  Utterances of n <= 128 take the
// short route further down: their eigensolver is the dense Jacobi solve, a workgroup per member,
// up to kShortWidth members per launch (run_short_route).  Results agree with
// sc_predict to the solver's tolerance (the grouped GEMMs sum whole K tiles, the group sets
// the check schedule), and a batch call is a deterministic function of its input.
// A batch may carry one speaker-turn band per utterance (sc_predict_batch_constrained): the same
// routes on one lane with member-by-member fronts, each member's band resident in its arena, and
// ConstraintPropagation before refinement as one chain of grouped launches per group
// (enqueue_front; constraint_api.hip: constraint_propagation_group).
#include <ctime>
#include <map>
#include <thread>
#include <utility>

#include "handle.h"

namespace {

double now_us() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}

constexpr int kRndStride = 256;  // doubles per k in the RandomState(0) table (k <= 32)

int group_slot(sc_handle lead, int z, sc_handle* out,
               std::vector<sc_handle_s*>* arenas = nullptr) {
  std::vector<sc_handle_s*>& slots = arenas ? *arenas : lead->gslots;
  while ((int)slots.size() <= z) {
    sc_handle sub = nullptr;
    const int rc = sc_create(lead->device, &sub);
    if (rc != SC_OK) return fail(lead, rc, "could not create a member arena for the group");
    // the member's stages before the eigensolver run on its own stream (several members'
    // GEMMs and refinement passes share the chip); `sync_ev` hands the result to the
    // owner's stream, where the lockstep chains run
    if (hipEventCreateWithFlags(&sub->sync_ev, hipEventDisableTiming) != hipSuccess) {
      sc_destroy(sub);
      return fail(lead, SC_ERR_HIP, "could not create a member event");
    }
    sub->profile_level = 1;
    slots.push_back(sub);
  }
  *out = slots[z];
  // (weights of a blur radius above 32 live in the handle: members inherit the lead's)
  if ((*out)->blur_ext.size() != lead->blur_ext.size() || !lead->blur_ext.empty())
    (*out)->blur_ext = lead->blur_ext;
  return SC_OK;
}

// A bank's stream and hand-over event, where the batch has not placed them on queues of their own
int ensure_bank_stream(sc_handle h, int b) {
  if (!h->gbank_stream[b])
    SC_HIP(h, hipStreamCreateWithFlags(&h->gbank_stream[b], hipStreamNonBlocking));
  if (!h->gbank_ev[b])
    SC_HIP(h, hipEventCreateWithFlags(&h->gbank_ev[b], hipEventDisableTiming));
  return SC_OK;
}

int ensure_seed_table(sc_handle lead) {
  if (lead->gkrnd_ready) return SC_OK;
  std::vector<double> table((size_t)33 * kRndStride, 0.0), rnd;
  for (int k = 1; k <= 32; ++k) {
    double u;
    int trials;
    kmeans_seed_constants(k, &u, &trials, &rnd);
    if (rnd.size() > (size_t)kRndStride) return fail(lead, SC_ERR_UNSUPPORTED, "seed table");
    std::copy(rnd.begin(), rnd.end(), table.begin() + (size_t)k * kRndStride);
  }
  SC_TRY(grow(lead, lead->gkrnd, table.size() * sizeof(double)));
  SC_HIP(lead, hipMemcpyAsync(lead->gkrnd.p, table.data(), table.size() * sizeof(double),
                              hipMemcpyHostToDevice, lead->stream));
  SC_HIP(lead, hipStreamSynchronize(lead->stream));  // `table` is a local
  lead->gkrnd_ready = true;
  return SC_OK;
}

struct Member {
  int index = -1;        // utterance
  sc_handle h = nullptr;
  FrontResult front;      // (front.free_op: matrix-free Diffuse, front.matrix is A)
  int state = 0;         // 0 in the group, 1 single-call path, 2 done
  int k = 0;
  const GroupEigMember* eig = nullptr;  // what the group's eigensolver left for it
};

// What a constrained batch carries (sc_predict_batch_constrained): per utterance the band of its
// ConstraintMatrix (host memory, n_i - 1 values; nullptr: that utterance has no constraint).
struct Bands {
  const double* const* band = nullptr;
  bool chain = false;  // ConstraintPropagation before refinement: the grouped Neumann chain
  int ncp = 0;         // cp[] work matrices a member arena holds for the configured operator
};
Bands make_bands(const double* const* band, const sc_config* cfg) {
  Bands b;
  if (cfg->constraint_name == SC_CONSTRAINT_NONE) return b;  // (nothing would read them)
  b.band = band;
  if (cfg->constraint_name == SC_CONSTRAINT_PROPAGATION) {
    b.chain = cfg->constraint_before_refinement != 0;
    // the grouped chain works in B1 / B2 (idle until refinement starts) + two more matrices; after
    // refinement the member's own constraint_propagation() takes its five
    b.ncp = b.chain ? 2 : 5;
  }
  return b;
}
// ... and what a member arena holds for it, reserved with the arena (never inside a front)
int reserve_constraint(sc_handle hz, const Bands* bands, int n_max) {
  if (!bands || !bands->band) return SC_OK;
  SC_TRY(grow(hz, hz->Cband, (size_t)std::max(n_max - 1, 1) * sizeof(double)));
  const size_t nn = (size_t)n_max * matrix_ld(n_max) * sizeof(double);
  for (int i = 0; i < bands->ncp; ++i) SC_TRY(grow(hz, hz->cp[i], nn));
  return SC_OK;
}

// Stages before the eigensolver of one group, member after member, each on its member's
// stream: no synchronisation.  `slot0`: first member arena of the bank the group uses.
// `arenas`: the member arenas to use (default: the lead's gslots).
// `bands`: a member's band goes up behind its affinity and becomes the arena's resident
// constraint; AffinityIntegration and the after-refinement operators then run per member as in a
// single call.  ConstraintPropagation before refinement is ONE grouped chain per 16 members on
// `chain_stream`: it waits for the members' affinities, `chain_ev` hands the adjusted affinities
// back to the member streams, which go on into the refinement.
int enqueue_front(sc_handle lead, const sc_array* xs, const int* ns, int d,
                  const sc_config* cfg, sc_diag* diags, const int* idx, int count, int slot0,
                  Member* mb, std::vector<sc_handle_s*>* arenas = nullptr,
                  const Bands* bands = nullptr, hipStream_t chain_stream = nullptr,
                  hipEvent_t chain_ev = nullptr) {
  // refinement, scaling vectors and the hand-over event of member z
  auto refine = [&](int z) -> int {
    Member& m = mb[z];
    sc_handle h = m.h;
    sc_diag local;
    sc_diag* dg = diags ? diags + m.index : &local;
    if (!diags) memset(&local, 0, sizeof(local));
    const int rc = eig_ncluster_impl(h, cfg, dg, &m.front);
    if (rc != SC_OK) {
      lead->err = h->err;
      return rc;
    }
    if (!m.front.symmetric) m.state = 1;
    SC_HIP(lead, hipEventRecord(h->sync_ev, h->stream));
    return SC_OK;
  };
  std::vector<int> chained;  // members whose affinity the grouped chain adjusts
  for (int z = 0; z < count; ++z) {
    Member& m = mb[z];
    m = Member();
    m.index = idx[z];
    SC_TRY(group_slot(lead, slot0 + z, &m.h, arenas));
    sc_handle h = m.h;
    h->err.clear();
    // (no wait: the caller's arrays stay valid for the whole batch call)
    int rc = ingest_embeddings(h, xs[m.index], false);
    h->nev = 0;
    if (diags) memset(diags + m.index, 0, sizeof(sc_diag));
    if (rc == SC_OK) rc = sc_compute_affinity(h);
    // the arena's resident constraint is this member's band, or none
    h->have_constraint = h->constraint_banded = false;
    h->qn = 0;
    const double* band = bands && bands->band ? bands->band[m.index] : nullptr;
    if (rc == SC_OK && band) {
      const size_t bytes = (size_t)(h->n - 1) * sizeof(double);
      rc = grow(h, h->Cband, std::max<size_t>(bytes, sizeof(double)));
      if (rc == SC_OK && bytes > 0 &&
          hipMemcpyAsync(h->Cband.p, band, bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess)
        rc = fail(h, SC_ERR_HIP, "could not upload a constraint band");
      h->have_constraint = h->constraint_banded = h->constraint_symmetric = true;
      h->qn = h->n;
    }
    if (rc == SC_OK && band && bands->chain) {
      chained.push_back(z);
      SC_HIP(lead, hipEventRecord(h->sync_ev, h->stream));  // "affinity and band are there"
      continue;
    }
    if (rc == SC_OK && constraint_active(h, cfg, true)) rc = sc_apply_constraint(h, cfg);
    if (rc != SC_OK) {
      lead->err = h->err;
      return rc;
    }
    SC_TRY(refine(z));
  }
  if (chained.empty()) return SC_OK;
  for (int z : chained) SC_HIP(lead, hipStreamWaitEvent(chain_stream, mb[z].h->sync_ev, 0));
  for (size_t at = 0; at < chained.size(); at += kGroupMax) {
    CpGroupMember cm[kGroupMax];
    const int cnt = (int)std::min<size_t>(kGroupMax, chained.size() - at);
    for (int q = 0; q < cnt; ++q) {
      sc_handle h = mb[chained[at + q]].h;
      const size_t nn = (size_t)h->n * h->ldn * sizeof(double);
      if (h->cp[0].bytes < nn || h->cp[1].bytes < nn || h->B1.bytes < nn || h->B2.bytes < nn)
        return fail(lead, SC_ERR_INVALID, "member arena without the chain's work matrices");
      cm[q].n = h->n;
      cm[q].ld = h->ldn;
      cm[q].A = ptr<double>(h->A0);
      cm[q].P = ptr<double>(h->B1);
      cm[q].T = ptr<double>(h->B2);
      cm[q].Pn = ptr<double>(h->cp[0]);
      cm[q].Tn = ptr<double>(h->cp[1]);
      cm[q].deg = ptr<double>(h->deg);
      cm[q].rowmax = ptr<double>(h->cut);
      cm[q].band = ptr<double>(h->Cband);
      cm[q].tilemap = h->tilemap_cur;
    }
    SC_TRY(constraint_propagation_group(lead, chain_stream, cm, cnt, cfg->constraint_alpha));
  }
  SC_HIP(lead, hipEventRecord(chain_ev, chain_stream));
  for (int z : chained) {
    sc_handle h = mb[z].h;
    SC_HIP(lead, hipStreamWaitEvent(h->stream, chain_ev, 0));
    h->have_cropval = false;  // (what sc_apply_constraint leaves: the epilogue's crop values are stale)
    h->constraint_applied = true;
    h->n_vec = 0;
    SC_TRY(refine(z));
  }
  return SC_OK;
}

// The ICASSP2018 sequence (CropDiagonal, GaussianBlur, RowWiseThreshold, Symmetrize, Diffuse,
// RowWiseNormalize with the fusions eig_ncluster_impl applies to it: crop value out of the
// affinity epilogue, blur with the diagonal override and per-strip row maxima, threshold +
// symmetrise in one pass, row statistics out of the Diffuse epilogue, RowWiseNormalize folded
// into the scaling vectors) is what the grouped front covers; anything else takes the
// member-by-member front above.
bool grouped_front_covers(const sc_config* cfg) {
  static const int seq[6] = {SC_OP_CROP_DIAGONAL, SC_OP_GAUSSIAN_BLUR, SC_OP_ROW_WISE_THRESHOLD,
                             SC_OP_SYMMETRIZE, SC_OP_DIFFUSE, SC_OP_ROW_WISE_NORMALIZE};
  if (cfg->n_ops != 6) return false;
  for (int i = 0; i < 6; ++i)
    if (cfg->ops[i] != seq[i]) return false;
  return (cfg->blur_radius == 4 || cfg->blur_radius == 8) &&
         cfg->threshold_type == SC_THRESHOLD_ROW_MAX && !cfg->preserve_diagonal;
}

// Stages before the eigensolver of one group as GROUPED launches on the bank's stream: the
// two GEMMs take the tiles of all members in one launch each (one utterance's 36..300 tiles
// cannot fill the chip, those of 16 can), the passes between them one launch each with
// blockIdx.y / z = member.  Same kernel bodies and arguments per member as
// sc_compute_affinity + eig_ncluster_impl; the GEMMs compute every tile whole (a single call
// splits the tiles of a short utterance over K: the sums differ in the last bits).
int enqueue_front_grouped(sc_handle lead, const sc_array* xs, const int* ns, int d,
                          const sc_config* cfg, sc_diag* diags, const int* idx, int count,
                          int slot0, Member* mb, int bank) {
  hipStream_t s = lead->gbank_stream[bank];
  FrontItem fi[kGroupMax];
  GemmGroupItem aff[kGroupMax], dif[kGroupMax];
  memset(fi, 0, sizeof(fi));
  for (int z = 0; z < count; ++z) {
    Member& m = mb[z];
    m = Member();
    m.index = idx[z];
    SC_TRY(group_slot(lead, slot0 + z, &m.h));
    sc_handle h = m.h;
    h->err.clear();
    const int n = ns[m.index];
    // the rows go in on the bank's stream, ahead of the front's launches (arena and problem
    // size are set by the same call)
    int rc = ingest_embeddings(h, xs[m.index], false, s);
    if (rc == SC_OK) rc = ensure_eig(h, n);
    if (rc == SC_OK) rc = ensure_tilemap(h, n);
    if (rc == SC_OK) rc = grow(h, h->symflag, 16);
    if (rc != SC_OK) {
      lead->err = h->err;
      return rc;
    }
    h->n = n;
    h->d = d;
    h->ldn = matrix_ld(n);
    h->ldx = round_up(d, 16);
    h->n_vec = 0;
    h->nev = 0;
    h->have_x = h->have_affinity = h->have_cropval = true;
    h->affinity_symmetric = h->affinity_from_embeddings = true;
    h->constraint_applied = false;
    if (diags) memset(diags + m.index, 0, sizeof(sc_diag));
    FrontItem& f = fi[z];
    f.X = ptr<double>(h->X);
    f.Xn = ptr<double>(h->Xn);
    f.ldx = h->ldx;
    f.n = n;
    f.d = d;
    f.ldn = h->ldn;
    f.A0 = ptr<double>(h->A0);
    f.B1 = ptr<double>(h->B1);
    f.B2 = ptr<double>(h->B2);
    f.cropval = ptr<double>(h->cropval);
    f.rmpart = ptr<double>(h->rmpart);
    f.blur_cols = blur_stream_columns(n, cfg->blur_radius);  // (the grouped front streams)
    f.cut = ptr<double>(h->cut);
    f.rowmax = ptr<double>(h->rowmax);
    f.rowsum = ptr<double>(h->rowsum);
    f.cvec = ptr<double>(h->cvec);
    f.pvec = ptr<double>(h->pvec);
    f.tvec = ptr<double>(h->tvec);
    f.symflag = ptr<int>(h->symflag);
    f.flags = ptr<int>(h->flags);
    const int nt = gemm_tile_dim(n);
    aff[z] = GemmGroupItem();
    aff[z].A = f.Xn;
    aff[z].lda = h->ldx;
    aff[z].C = f.A0;
    aff[z].ldc = h->ldn;
    aff[z].n = n;
    aff[z].K = d;
    aff[z].tilemap = h->tilemap_cur;
    aff[z].partial_max = ptr<double>(h->statp);
    aff[z].rowmax = ptr<double>(h->cropval);
    m.front.crop_source = 1;  // (the affinity epilogue writes the value the blur reads)
    dif[z] = GemmGroupItem();
    dif[z].A = f.B2;
    dif[z].lda = h->ldn;
    dif[z].C = f.B1;
    dif[z].ldc = h->ldn;
    dif[z].n = n;
    dif[z].K = n;
    dif[z].tilemap = h->tilemap_cur;
    dif[z].partial_max = ptr<double>(h->statp);
    dif[z].partial_sum = ptr<double>(h->statp) + (size_t)n * nt;
    dif[z].rowmax = ptr<double>(h->rowmax);
    dif[z].rowsum = ptr<double>(h->rowsum);
    m.front.matrix = f.B1;
    m.front.scratch = f.B2;
    m.front.ld = h->ldn;
    m.front.symmetric = true;
    m.front.folded_rownorm = true;
    // Large members take the matrix-free Diffuse (free_api.hip): their n^3 product is most of
    // a batch's GEMM time (78 % of config 5's Diffuse flops sit in utterances of n >= 2048;
    // members switch from n = 1536 on: free_diffuse_wanted).  (A hand-back resumes on the
    // two-pass operator: api.hip.)
    m.front.free_op = free_diffuse_wanted(lead, cfg, n, make_eig_request(cfg), true) &&
                      cfg->soft_multiplier >= 0.0 && cfg->soft_multiplier <= 1.0 &&
                      cfg->p_percentile > 0.0;
    if (m.front.free_op) {
      rc = ensure_free(h, n);
      if (rc != SC_OK) {
        lead->err = h->err;
        return rc;
      }
      dif[z].n = 0;          // idle in the grouped fp64 product
      m.front.matrix = f.B2;  // the thresholded + symmetrised A stays the operand
      m.front.scratch = f.B1;
    }
  }
  launch_front_begin_group(s, fi, count, true);
  launch_gemm_nt_group(s, aff, count, kEpiAffinity, 2);
  launch_gaussian_blur_group(s, fi, count, cfg->blur_radius, ptr<double>(lead->blurw),
                             &lead->last_blur);
  // rowmax / rowsum of S = A A^T without forming it, for the members that take that route (the
  // cut vector bounds max|a|: the grouped front is the ICASSP2018 sequence on a cosine affinity):
  // begin, scan and statistics are one launch each for all of them, the digit products one
  // launch with a member per blockIdx.y; round 6: their digits come out of the threshold pass
  sc_handle fh[kGroupMax];
  const double* mats[kGroupMax];
  const double* cuts[kGroupMax];
  double ps[kGroupMax];
  int nn[kGroupMax], ll[kGroupMax], nf = 0, fz[kGroupMax];
  FreeItem fitems[kGroupMax];
  for (int z = 0; z < count; ++z) {
    if (!mb[z].front.free_op) continue;
    sc_handle h = mb[z].h;
    fh[nf] = h;
    fz[nf] = z;
    mats[nf] = fi[z].B2;
    cuts[nf] = ptr<double>(h->cut);
    ps[nf] = cfg->p_percentile;
    nn[nf] = h->n;
    ll[nf] = h->ldn;
    ++nf;
  }
  if (nf > 0) {
    // (the cuts first -- max|a| comes from them --, then the begin step, then the pass itself)
    launch_cut_from_partials_group(s, fi, count, cfg->p_percentile);
    TsDigits packed[kGroupMax], digits[kGroupMax];
    memset(digits, 0, sizeof(digits));
    const double amax_floor = (cfg->binarize || cfg->preserve_diagonal) ? 1.0 : 0.0;
    SC_TRY(free_group_prepare(fh, mats, cuts, ps, nf, ll, nn, s, amax_floor, fitems, packed));
    for (int q = 0; q < nf; ++q) digits[fz[q]] = packed[q];
    launch_threshold_symmetrize_group(s, fi, count, cfg->p_percentile, cfg->soft_multiplier,
                                      cfg->binarize, cfg->symmetrize_type, cfg->preserve_diagonal,
                                      true, digits);
    for (int z = 0; z < count; ++z) mb[z].front.digits_fused = digits[z].Q != nullptr;
  } else {
    // (the cuts come from the blur's partials inside this launcher)
    launch_threshold_symmetrize_group(s, fi, count, cfg->p_percentile, cfg->soft_multiplier,
                                      cfg->binarize, cfg->symmetrize_type, cfg->preserve_diagonal);
  }
  for (int z = 0; z < count; ++z) mb[z].front.cut_kernel = 1;  // k_cut_from_partials_g either way
  for (int z = 0; z < count; ++z) mb[z].front.diffuse_explicit = dif[z].n > 0;
  launch_gemm_nt_group(s, dif, count, kEpiNone, 1);
  if (nf > 0) {
    SC_TRY(free_group_digits(fh, fitems, nf, s));
    {  // the digit products of all of them: one launch (blockIdx.y = member)
      const signed char* qs[kGroupMax];
      float* ts[kGroupMax];
      unsigned* ms[kGroupMax];
      const int2* tms[kGroupMax];
      const int* pls[kGroupMax];
      for (int q = 0; q < nf; ++q) {
        qs[q] = ptr<signed char>(fh[q]->fq);
        ts[q] = ptr<float>(fh[q]->ft32);
        ms[q] = ptr<unsigned>(fh[q]->fwords);
        tms[q] = fh[q]->tilemap_cur;
        pls[q] = fitems[q].plan;
      }
      launch_gemm_i8_sym_group(s, qs, ts, ms, nf, nn, tms, pls);
    }
    SC_TRY(free_group_end(fh, fitems, nf, s));
  }
  launch_scaling_vectors_group(s, fi, count, cfg->laplacian_type, 1);
  SC_TRY(check_last(lead, "grouped front launch"));
  SC_HIP(lead, hipEventRecord(lead->gbank_ev[bank], s));
  return SC_OK;
}

// What the wave front of the short route covers: an in-order CropDiagonal, GaussianBlur (weights
// in the config: radius <= 32), then RowWiseThreshold + Symmetrize (every option of the two),
// optionally Diffuse, optionally a last RowWiseNormalize, which folds into the scaling vectors.
// The result is symmetric by construction.  (Sequences without the threshold + symmetrise pair
// keep the member-by-member front.)
bool short_wave_covers(const sc_config* cfg, ShortWaveOps* ops) {
  ShortWaveOps o;
  memset(&o, 0, sizeof(o));
  int i = 0;
  auto take = [&](int op) { return i < cfg->n_ops && cfg->ops[i] == op ? (++i, true) : false; };
  o.crop = take(SC_OP_CROP_DIAGONAL);
  if (take(SC_OP_GAUSSIAN_BLUR)) {
    if (cfg->blur_radius > SC_MAX_BLUR_RADIUS) return false;
    o.blur_radius = cfg->blur_radius;  // (0: gaussian_filter degenerates to a copy)
  }
  if (!take(SC_OP_ROW_WISE_THRESHOLD) || !take(SC_OP_SYMMETRIZE)) return false;
  o.diffuse = take(SC_OP_DIFFUSE);
  o.rownorm = take(SC_OP_ROW_WISE_NORMALIZE);
  if (i != cfg->n_ops) return false;
  o.threshold_type = cfg->threshold_type;
  o.binarize = cfg->binarize;
  o.symtype = cfg->symmetrize_type;
  o.preserve_diag = cfg->preserve_diagonal;
  o.p = cfg->p_percentile;
  o.mult = cfg->soft_multiplier;
  o.lap = cfg->laplacian_type;
  if (ops) *ops = o;
  return true;
}
// d <= kShortWaveMaxD: a single call of n <= 128 runs its affinity product as whole-K tiles
// (gemm_f64.hip launch_variant: "if (K <= 512 && full == 0) ksplit = 1"), which is what the
// grouped product computes -- the wave front's bits are then the single call's.  The Diffuse
// product has K = n <= 128.
constexpr int kShortWaveMaxD = 512;

// Stages before the eigensolver of one WAVE of the short route (up to kShortWidth members of
// n <= kDenseMax) on the bank's stream: the row normalisation and the two GEMMs through the group
// launchers, kGroupMax members per launch; everything between them ONE launch for the wave
// (k_short_wave_front, a workgroup per member), descriptors from a table that goes up in one copy
// (half `bank` of lead->gswtab).  3 ceil(count / 16) + 3 kernel launches with a Diffuse,
// 2 ceil(count / 16) + 2 without, besides the members' ingest.  Per member the values a single
// call stores (tests/test_gpu_short_wave_front.py).
int enqueue_front_short_wave(sc_handle lead, const sc_array* xs, const int* ns, int d,
                             const sc_config* cfg, sc_diag* diags, const int* idx, int count,
                             int slot0, Member* mb, int bank, const ShortWaveOps& ops) {
  hipStream_t s = lead->gbank_stream[bank];
  const size_t half = (size_t)kShortWidth * sizeof(ShortWaveItem);
  SC_TRY(grow(lead, lead->gswtab, kGroupBanks * half));
  if (!lead->h_gswtab)
    SC_HIP(lead, hipHostMalloc(reinterpret_cast<void**>(&lead->h_gswtab), kGroupBanks * half));
  // (the pinned half is rewritten: the wave that used it last has been solved, its copy read)
  ShortWaveItem* htab = lead->h_gswtab + (size_t)bank * kShortWidth;
  ShortWaveItem* dtab = ptr<ShortWaveItem>(lead->gswtab) + (size_t)bank * kShortWidth;
  std::vector<FrontItem> fi(count);
  std::vector<GemmGroupItem> aff(count), dif(count);
  memset(fi.data(), 0, fi.size() * sizeof(FrontItem));
  for (int z = 0; z < count; ++z) {
    Member& m = mb[z];
    m = Member();
    m.index = idx[z];
    SC_TRY(group_slot(lead, slot0 + z, &m.h, &lead->gshort));
    sc_handle h = m.h;
    h->err.clear();
    const int n = ns[m.index];
    if (n > kDenseMax) return fail(lead, SC_ERR_INVALID, "short wave: a member above 128 rows");
    int rc = ingest_embeddings(h, xs[m.index], false, s);
    if (rc == SC_OK) rc = ensure_eig(h, n);
    if (rc == SC_OK) rc = ensure_tilemap(h, n);
    if (rc == SC_OK) rc = grow(h, h->symflag, 16);
    if (rc != SC_OK) {
      lead->err = h->err;
      return rc;
    }
    h->n = n;
    h->d = d;
    h->ldn = matrix_ld(n);
    h->ldx = round_up(d, 16);
    h->n_vec = 0;
    h->nev = 0;
    h->have_x = h->have_affinity = true;
    h->have_cropval = ops.crop != 0;  // (the front kernel writes the vector only then)
    h->affinity_symmetric = h->affinity_from_embeddings = true;
    h->constraint_applied = false;
    h->have_constraint = h->constraint_banded = false;
    h->qn = 0;
    if (diags) memset(diags + m.index, 0, sizeof(sc_diag));
    FrontItem& f = fi[z];
    f.X = ptr<double>(h->X);
    f.Xn = ptr<double>(h->Xn);
    f.ldx = h->ldx;
    f.n = n;
    f.d = d;
    f.ldn = h->ldn;
    f.symflag = ptr<int>(h->symflag);
    f.flags = ptr<int>(h->flags);
    aff[z] = GemmGroupItem();
    aff[z].A = f.Xn;
    aff[z].lda = h->ldx;
    aff[z].C = ptr<double>(h->A0);
    aff[z].ldc = h->ldn;
    aff[z].n = n;
    aff[z].K = d;
    aff[z].tilemap = h->tilemap_cur;
    aff[z].partial_max = ptr<double>(h->statp);
    dif[z] = GemmGroupItem();
    dif[z].A = ptr<double>(h->B2);
    dif[z].lda = h->ldn;
    dif[z].C = ptr<double>(h->B1);
    dif[z].ldc = h->ldn;
    dif[z].n = n;
    dif[z].K = n;
    dif[z].tilemap = h->tilemap_cur;
    dif[z].partial_max = ptr<double>(h->statp);
    dif[z].partial_sum = ptr<double>(h->statp) + n;  // (one tile: gemm_tile_dim(n) = 1)
    ShortWaveItem& it = htab[z];
    it.n = n;
    it.ld = h->ldn;
    it.a0 = ptr<double>(h->A0);
    it.stat0 = ptr<double>(h->statp);
    it.cropval = ptr<double>(h->cropval);
    it.out = ptr<double>(h->B2);
    it.cut = ptr<double>(h->cut);
    it.stat1 = ptr<double>(h->statp);
    it.rowmax = ptr<double>(h->rowmax);
    it.rowsum = ptr<double>(h->rowsum);
    it.cvec = ptr<double>(h->cvec);
    it.pvec = ptr<double>(h->pvec);
    it.tvec = ptr<double>(h->tvec);
    it.flags = ptr<int>(h->flags);
    it.symflag = ptr<int>(h->symflag);
    m.front.matrix = ops.diffuse ? ptr<double>(h->B1) : ptr<double>(h->B2);
    m.front.scratch = ops.diffuse ? ptr<double>(h->B2) : ptr<double>(h->B1);
    m.front.ld = h->ldn;
    m.front.symmetric = true;
    m.front.folded_rownorm = ops.rownorm != 0;
    m.front.laplacian_type = cfg->laplacian_type;
    m.front.chain_flags_cleared = true;
    m.front.diffuse_explicit = ops.diffuse != 0;
    m.front.crop_source = ops.crop ? 1 : 0;  // (the affinity epilogue's partials)
    m.front.cut_kernel = 5;                  // k_short_wave_front
  }
  int launches = 0;
  SC_HIP(lead, hipMemcpyAsync(dtab, htab, (size_t)count * sizeof(ShortWaveItem),
                              hipMemcpyHostToDevice, s));
  launch_short_wave_init(s, dtab, count);
  ++launches;
  for (int at = 0; at < count; at += kGroupMax) {
    const int c = std::min(kGroupMax, count - at);
    launch_front_begin_group(s, fi.data() + at, c, true, false);
    launch_gemm_nt_group(s, aff.data() + at, c, kEpiAffinity, 2, false);
    launches += 2;
  }
  launch_short_wave_front(s, dtab, count, ops, ptr<double>(lead->blurw));
  ++launches;
  if (ops.diffuse) {
    for (int at = 0; at < count; at += kGroupMax) {
      launch_gemm_nt_group(s, dif.data() + at, std::min(kGroupMax, count - at), kEpiNone, 1, false);
      ++launches;
    }
    launch_short_wave_scaling(s, dtab, count, cfg->laplacian_type, ops.rownorm);
    ++launches;
  }
  lead->gsw_launches = launches;
  SC_TRY(check_last(lead, "short wave front launch"));
  SC_HIP(lead, hipEventRecord(lead->gbank_ev[bank], s));
  return SC_OK;
}

// k-means of up to kGroupMax members whose eigensolver has finished (mb[zs[e]].eig), in lockstep
// on the owner's stream, and their labels; both routes of the grouped batch end here.  A member
// whose solve or cluster count left the common path gets state 1 (single_path_members below).
// `eig_path` / `route`: what the members' diagnostics and route codes report.
int cluster_members(sc_handle lead, const int* ns, const sc_config* cfg, int64_t* const* labels,
                    sc_diag* diags, Member* mb, const int* zs, int nz, const EigRequest& rq,
                    int eig_path, int route, int* clustered) {
  hipStream_t s = lead->stream;
  KmGroupItem km[kGroupMax];
  int kmz[kGroupMax], label_n[kGroupMax];
  size_t label_off[kGroupMax], label_total = 0;
  int nk = 0;
  {  // staging for the labels of these members (every one of them could end up in it)
    size_t need = 0;
    for (int e = 0; e < nz; ++e) need += (size_t)ns[mb[zs[e]].index];
    // (never less than a full group of the largest utterances the grouped path takes -- 512 KB:
    //  a staging buffer that follows the batch's composition is a hipHostFree + hipHostMalloc,
    //  milliseconds, whenever a group's total grows)
    need = std::max(need, (size_t)kGroupMax * 4096);
    SC_TRY(grow(lead, lead->ginfo, (size_t)kGroupMax * 16 * sizeof(int)));
    SC_TRY(grow(lead, lead->glabels, need * sizeof(int64_t)));
    if (!lead->h_ginfo)
      SC_HIP(lead, hipHostMalloc(reinterpret_cast<void**>(&lead->h_ginfo),
                                 (size_t)kGroupMax * 16 * sizeof(int)));
    if (lead->h_glabels_count < need) {
      if (lead->h_glabels) SC_HIP(lead, hipHostFree(lead->h_glabels));
      lead->h_glabels = nullptr;
      lead->h_glabels_count = 0;
      SC_HIP(lead, hipHostMalloc(reinterpret_cast<void**>(&lead->h_glabels),
                                 need * sizeof(int64_t)));
      lead->h_glabels_count = need;
    }
  }
  for (int e = 0; e < nz; ++e) {
    Member& m = mb[zs[e]];
    const GroupEigMember& g = *m.eig;
    if (g.status != 0) {
      m.state = 1;
      m.front.skip_fused = g.skip_fused;  // (what the resumed single-call solve starts from)
      continue;
    }
    sc_handle h = m.h;
    const int n = g.n;
    int k = g.dc.n_clusters_raw;
    if (cfg->min_clusters > 0 && k < cfg->min_clusters) k = cfg->min_clusters;  // :295-296
    m.k = k;
    double u = 0.0;
    int trials = 0;
    std::vector<double> unused;
    if (k >= 1 && k <= 32) kmeans_seed_constants(k, &u, &trials, &unused);
    if (k < 1 || k > 32 || k > h->n_vec || n < k || cfg->max_iter <= 0 ||
        !kmeans_chain_supported(n, k, trials) || sw::kmeans_single()) {
      m.state = 1;  // the single-call path states the error or takes the other kernel
      continue;
    }
    if (diags) {
      sc_diag* dg = diags + m.index;
      dg->n = n;
      dg->n_clusters_raw = g.dc.n_clusters_raw;
      dg->max_delta = g.dc.max_delta;
      dg->eig_descending = rq.descend;
      dg->n_eigenvalues = std::min((int)g.w.size(), SC_MAX_EIG);
      for (int i = 0; i < dg->n_eigenvalues; ++i) dg->eigenvalues[i] = g.w[i];
      dg->symmetry_state = m.front.folded_rownorm ? 2 : 1;
      dg->eig_path = eig_path;
      dg->eig_matvec_passes = g.passes;
      dg->eig_block = kEigBlock;
      dg->eig_basis = g.basis;
      dg->eig_max_residual = g.dc.max_resid;
      dg->n_clusters = k;
      if (m.front.free_op) {
        dg->diffuse_path = SC_DIFFUSE_PATH_FREE;
        dg->free_candidates = h->h_free[65];
        dg->free_tiles_run = h->h_free[67];
      } else if (m.front.folded_rownorm) {  // (the grouped front: the explicit product)
        dg->diffuse_path = SC_DIFFUSE_PATH_EXPLICIT;
      }
    }
    SC_TRY(ensure_kmeans(h, n));
    const int lde = round_up(n, 16);
    const double* E = ptr<double>(h->E);
    if (cfg->row_wise_renorm) {
      SC_HIP(lead, hipMemcpyAsync(h->Ek.p, h->E.p, (size_t)lde * k * sizeof(double),
                                  hipMemcpyDeviceToDevice, s));
      launch_row_renorm(s, ptr<double>(h->Ek), lde, n, k);
      E = ptr<double>(h->Ek);
    }
    KmGroupItem& it = km[nk];
    it = KmGroupItem();
    it.ET = E;
    it.lde = lde;
    it.n = n;
    it.k = k;
    it.max_iter = cfg->max_iter;
    it.first_center = sc_uniform_choice(n, u);
    it.trials = trials;
    it.ws = kmeans_workspace(h);
    it.ws.rnd = ptr<double>(lead->gkrnd) + (size_t)k * kRndStride;
    // the stop words and the labels of the whole group live side by side: one copy each
    it.ws.info = ptr<int>(lead->ginfo) + 16 * nk;
    it.ws.labels64 = ptr<long long>(lead->glabels) + label_total;
    label_off[nk] = label_total;
    label_total += (size_t)n;
    kmz[nk++] = zs[e];
  }
  int running = nk;
  for (int it = 0; running > 0; it += 4) {
    launch_kmeans_chain_group(s, km, nk, it, 4);
    SC_TRY(check_last(lead, "group kmeans launch"));
    SC_HIP(lead, hipMemcpyAsync(lead->h_ginfo, lead->ginfo.p, (size_t)nk * 16 * sizeof(int),
                                hipMemcpyDeviceToHost, s));
    SC_HIP(lead, hipStreamSynchronize(s));
    for (int q = 0; q < nk; ++q) {
      if (km[q].n <= 0 || lead->h_ginfo[16 * q + 8] == 0) continue;
      Member& m = mb[kmz[q]];
      if (diags) diags[m.index].kmeans_iterations = lead->h_ginfo[16 * q];
      m.state = 2;
      if (lead->groutes) lead->groutes[m.index] = route;
      label_n[q] = km[q].n;
      km[q].n = 0;  // idle from here on
      --running;
    }
    if (running > 0 && it > cfg->max_iter + 4)
      return fail(lead, SC_ERR_HIP, "k-means chain did not reach its stop rule");
  }
  if (nk > 0) {
    SC_HIP(lead, hipMemcpyAsync(lead->h_glabels, lead->glabels.p, label_total * sizeof(int64_t),
                                hipMemcpyDeviceToHost, s));
    SC_HIP(lead, hipStreamSynchronize(s));
    for (int q = 0; q < nk; ++q)
      memcpy(labels[mb[kmz[q]].index], lead->h_glabels + label_off[q],
             (size_t)label_n[q] * sizeof(int64_t));
  }
  if (clustered) *clustered = nk;
  return SC_OK;
}

// The members of a group that left the common path (state 1): the single-call pipeline on their
// own arena, from the refined matrix their front left -- only the solver and k-means again.
int single_path_members(sc_handle lead, const sc_config* cfg, int64_t* const* labels,
                        sc_diag* diags, Member* mb, int count) {
  bool any_back = false;
  for (int z = 0; z < count; ++z) any_back = any_back || mb[z].state == 1;
  // (their speculative block steps may still be running on this stream)
  if (any_back) SC_HIP(lead, hipStreamSynchronize(lead->stream));
  for (int z = 0; z < count; ++z) {
    Member& m = mb[z];
    if (m.state != 1) continue;
    sc_diag local;
    sc_diag* dg = diags ? diags + m.index : &local;
    memset(dg, 0, sizeof(*dg));
    m.h->nev = 0;
    int rc = eig_ncluster_impl(m.h, cfg, dg, nullptr, &m.front);
    if (rc == SC_OK) {
      int k = dg->n_clusters_raw;
      if (cfg->min_clusters > 0 && k < cfg->min_clusters) k = cfg->min_clusters;  // :295-296
      rc = sc_cluster(m.h, cfg, k, labels[m.index], dg);
    }
    if (rc != SC_OK) {
      lead->err = m.h->err;
      return rc;
    }
  }
  return SC_OK;
}

// Eigensolver and k-means of a group whose stages before are enqueued (enqueue_front), in
// lockstep on the owner's stream; then the members that left the common path.
int finish_group(sc_handle lead, const int* ns, const sc_config* cfg, int64_t* const* labels,
                 sc_diag* diags, Member* mb, int count, const EigRequest& rq, int front_bank) {
  hipStream_t s = lead->stream;
  const bool trace = sw::group_trace();
  if (front_bank >= 0) {
    SC_HIP(lead, hipStreamWaitEvent(s, lead->gbank_ev[front_bank], 0));
  } else {
    for (int z = 0; z < count; ++z) SC_HIP(lead, hipStreamWaitEvent(s, mb[z].h->sync_ev, 0));
  }
  const double t1 = trace ? now_us() : 0.0;
  // ---- eigen: lockstep over the symmetric members
  GroupEigMember em[kGroupMax];
  int emz[kGroupMax], ne = 0;
  for (int z = 0; z < count; ++z) {
    if (mb[z].state != 0) continue;
    em[ne].h = mb[z].h;
    em[ne].S = mb[z].front.matrix;
    em[ne].ld = mb[z].front.ld;
    em[ne].n = ns[mb[z].index];
    em[ne].rq = rq;
    em[ne].free_op = mb[z].front.free_op;
    mb[z].eig = &em[ne];
    emz[ne++] = z;
  }
  if (ne > 0) SC_TRY(sym_topk_group(lead, em, ne));
  for (int e = 0; e < ne; ++e) {
    // a matrix-free member with rows the candidate search could not prune: the single-call
    // path evaluates those rows exactly (its overflow words came back with the solver's syncs;
    // eig_ncluster_impl's resume branch turns the two-pass operator back on: front.free_op)
    if (em[e].free_op && em[e].status == 0 && em[e].h->h_free[0] != 0) em[e].status = 1;
  }
  const double t2 = trace ? now_us() : 0.0;
  // ---- k-means: lockstep over the solved members
  int nk = 0;
  SC_TRY(cluster_members(lead, ns, cfg, labels, diags, mb, emz, ne, rq, SC_EIG_PATH_BLOCK_LANCZOS,
                         SC_BATCH_ROUTE_GROUP_LANCZOS, &nk));
  if (trace)
    fprintf(stderr, "[sc] group of %d (n %d..%d): eigen %.0f us, k-means %.0f us (%d members)\n",
            count, ns[mb[count - 1].index], ns[mb[0].index], t2 - t1, now_us() - t2, nk);
  // ---- members that left the common path: the single-call pipeline on their own arena
  return single_path_members(lead, cfg, labels, diags, mb, count);
}

// ------------------------------------------------------------------------------
// short route: n <= kDenseMax
// ------------------------------------------------------------------------------
// An utterance of n <= 128 ends in the one-workgroup Jacobi solve -- 1.7 .. 6.4 ms on ONE CU at
// n = 80 .. 128, longer than a whole call at n = 8192 -- and a batch of such utterances ran them
// one after the other.  Here a wave of up to kShortWidth of them shares ONE Jacobi launch, a
// workgroup (a CU) each (eig_driver.hip: dense_topk_group), and then the lockstep k-means chain
// of the grouped route, kGroupMax members at a time.  The front of a wave is enqueued one wave
// ahead of the wave being solved: ONE chain of launches for the wave on its bank's stream
// (enqueue_front_short_wave) when the batch has no constraint bands, d <= 512 and the refinement
// sequence is one short_wave_covers() names; else the single call's front, member by member on the
// member's stream (also with SC_SHORT_FRONT_MEMBERWISE=1).  Same kernel bodies and arguments per
// member as its own sc_predict (eigenvalues within 1e-10 relative; the wave front's bits are the
// single call's).
// Eigensolver and k-means of one wave whose fronts are enqueued:
int finish_short_wave(sc_handle lead, const int* ns, const sc_config* cfg, int64_t* const* labels,
                      sc_diag* diags, Member* mb, int count, const EigRequest& rq,
                      GroupEigMember* em, int front_bank = -1) {
  hipStream_t s = lead->stream;
  const bool trace = sw::group_trace();
  if (front_bank >= 0) {  // the wave front: one event for the wave
    SC_HIP(lead, hipStreamWaitEvent(s, lead->gbank_ev[front_bank], 0));
  } else {
    for (int z = 0; z < count; ++z) SC_HIP(lead, hipStreamWaitEvent(s, mb[z].h->sync_ev, 0));
  }
  const double t1 = trace ? now_us() : 0.0;
  std::vector<int> emz;
  for (int z = 0; z < count; ++z) {
    if (mb[z].state != 0) continue;  // (a front that is not symmetric: the general solver)
    GroupEigMember& g = em[emz.size()];
    g = GroupEigMember();
    g.h = mb[z].h;
    g.S = mb[z].front.matrix;
    g.ld = mb[z].front.ld;
    g.n = ns[mb[z].index];
    g.rq = rq;
    mb[z].eig = &g;
    emz.push_back(z);
  }
  const int ne = (int)emz.size();
  if (ne > 0) SC_TRY(dense_topk_group(lead, em, ne));
  const double t2 = trace ? now_us() : 0.0;
  int total = 0;
  for (int at = 0; at < ne; at += kGroupMax) {
    int nk = 0;
    SC_TRY(cluster_members(lead, ns, cfg, labels, diags, mb, emz.data() + at,
                           std::min(kGroupMax, ne - at), rq, SC_EIG_PATH_DENSE_JACOBI,
                           SC_BATCH_ROUTE_GROUP_JACOBI, &nk));
    total += nk;
  }
  if (trace)
    fprintf(stderr, "[sc] short wave of %d (n %d..%d): eigen %.0f us, k-means %.0f us (%d members)\n",
            count, ns[mb[count - 1].index], ns[mb[0].index], t2 - t1, now_us() - t2, total);
  return single_path_members(lead, cfg, labels, diags, mb, count);
}

int upload_group_blur_weights(sc_handle h, const sc_config* cfg);  // (further down)
// The short members of a batch (`list`: indices sorted by n, descending) in waves of kShortWidth
// on the caller's handle and host thread.
int run_short_route(sc_handle h, const sc_array* xs, const int* ns, int d,
                    const sc_config* cfg, int64_t* const* labels, sc_diag* diags,
                    const std::vector<int>& list, const EigRequest& rq, const Bands* bands) {
  if (list.empty()) return SC_OK;
  SC_HIP(h, hipStreamSynchronize(h->stream));
  SC_TRY(ensure_seed_table(h));
  const int total = (int)list.size();
  const int nwaves = (total + kShortWidth - 1) / kShortWidth;
  const int banks = std::min(kGroupBanks, nwaves);
  auto wave_count = [&](int j) { return std::min(kShortWidth, total - j * kShortWidth); };
  // arenas once, every one for n = kDenseMax (1 MB or so): a position takes a member of any
  // size of this route, and none of them ever holds a longer utterance of the batch
  for (int b = 0; b < banks; ++b)
    for (int z = 0; z < wave_count(b); ++z) {
      sc_handle hz = nullptr;
      SC_TRY(group_slot(h, b * kShortWidth + z, &hz, &h->gshort));
      int rc = sc_reserve(hz, kDenseMax, d);
      if (rc == SC_OK) rc = reserve_constraint(hz, bands, kDenseMax);
      if (rc != SC_OK) return fail(h, rc, hz->err);
      hz->have_constraint = false;
    }
  ShortWaveOps wave_ops;
  const bool wave = !sw::short_front_memberwise() && !(bands && bands->band) &&
                    d <= kShortWaveMaxD && short_wave_covers(cfg, &wave_ops);
  if (wave || (bands && bands->chain))  // (the grouped chain of a wave: a stream of the wave's bank)
    for (int b = 0; b < banks; ++b) SC_TRY(ensure_bank_stream(h, b));
  if (wave && wave_ops.blur_radius > 0) SC_TRY(upload_group_blur_weights(h, cfg));
  std::vector<Member> mbs[kGroupBanks];
  std::vector<GroupEigMember> em(kShortWidth);
  for (int b = 0; b < banks; ++b) mbs[b].resize(kShortWidth);
  auto front = [&](int j) -> int {
    if (wave)
      return enqueue_front_short_wave(h, xs, ns, d, cfg, diags,
                                      list.data() + (size_t)j * kShortWidth, wave_count(j),
                                      (j % banks) * kShortWidth, mbs[j % banks].data(), j % banks,
                                      wave_ops);
    return enqueue_front(h, xs, ns, d, cfg, diags, list.data() + (size_t)j * kShortWidth,
                         wave_count(j), (j % banks) * kShortWidth, mbs[j % banks].data(),
                         &h->gshort, bands, h->gbank_stream[j % banks], h->gbank_ev[j % banks]);
  };
  int rc = front(0);
  for (int j = 0; j < nwaves && rc == SC_OK; ++j) {
    bool ahead = false;
    if (j + 1 < nwaves) {
      rc = front(j + 1);
      ahead = true;
    }
    if (rc == SC_OK)
      rc = finish_short_wave(h, ns, cfg, labels, diags, mbs[j % banks].data(), wave_count(j), rq,
                             em.data(), wave ? j % banks : -1);
    if (rc != SC_OK && ahead) {  // the next wave's uploads read the caller's arrays: let them land
      if (wave) (void)hipStreamSynchronize(h->gbank_stream[(j + 1) % banks]);
      for (int z = 0; !wave && z < wave_count(j + 1); ++z)
        if (mbs[(j + 1) % banks][z].h) (void)hipStreamSynchronize(mbs[(j + 1) % banks][z].h->stream);
    }
  }
  return rc;
}

// ---- streams on hardware queues of their own
// The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (4 by
// default; the library does not touch the process environment -- a caller may export 8 before
// its first HIP call, api.hip / INTEGRATION.md section 4; round 5's probe measured 5950-6280
// utterances/s on config 5 with the default 4 and 5750-6120 with 8: no longer a difference),
// and streams that share a queue run one after the other.  A chain's 10 us launches queued behind a front's multi-millisecond GEMM cost
// a two-lane batch 10 % (3700 instead of 4100 utterances/s on config 5) whenever the creation
// order of the process's streams (every member arena owns one, an application has its own) put
// them together.  Which queue a new stream lands on is the runtime's business (ROCm 7.2: up
// the queues, then down again -- streams created back to back do collide where it turns), so
// it is MEASURED: a one-lane kernel spins for 150 us on stream a; a marker recorded on stream
// b right after it completes at once unless b sits behind a.
__global__ void k_spin(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) {}
}
int streams_share_queue(sc_handle h, hipStream_t a, hipStream_t b, hipEvent_t ea, hipEvent_t eb,
                        bool* share) {
  SC_HIP(h, hipStreamSynchronize(a));
  SC_HIP(h, hipStreamSynchronize(b));
  hipLaunchKernelGGL(k_spin, dim3(1), dim3(1), 0, a, 15000LL);  // 100 MHz ticks
  SC_HIP(h, hipEventRecord(ea, a));
  SC_HIP(h, hipEventRecord(eb, b));
  SC_HIP(h, hipEventSynchronize(eb));
  *share = hipEventQuery(ea) == hipSuccess;  // the spin was over before b's marker came through
  SC_HIP(h, hipStreamSynchronize(a));
  return SC_OK;
}
// Fills slots[0..count) with new streams none of which shares a hardware queue with another or
// with one of `have`; candidates that do are destroyed.  When the queues run out (a runtime
// initialised with 4 of them) the remaining slots take what comes -- the first slots, the
// chains, have been served by then.
int independent_streams(sc_handle h, std::vector<hipStream_t> have, hipStream_t** slots,
                        int count) {
  hipEvent_t ea = nullptr, eb = nullptr;
  SC_HIP(h, hipEventCreateWithFlags(&ea, hipEventDisableTiming));
  SC_HIP(h, hipEventCreateWithFlags(&eb, hipEventDisableTiming));
  std::vector<hipStream_t> rejected;
  int filled = 0, rc = SC_OK;
  for (int tries = 0; filled < count && tries < 4 * count + 16 && rc == SC_OK; ++tries) {
    hipStream_t cand = nullptr;
    // (one priority for all of them: a lower one for the banks, so that the short kernels of
    //  the chains go first, cost 8 %, a higher one 11 % -- the GEMMs are the throughput)
    if (hipStreamCreateWithPriority(&cand, hipStreamNonBlocking, 0) != hipSuccess) {
      rc = fail(h, SC_ERR_HIP, "could not create a stream for the grouped batch");
      break;
    }
    bool clash = false;
    for (size_t i = 0; i < have.size() && !clash && rc == SC_OK; ++i)
      rc = streams_share_queue(h, have[i], cand, ea, eb, &clash);
    if (rc != SC_OK || clash) {
      rejected.push_back(cand);  // (kept until the end: destroying it now would free its place)
      continue;
    }
    have.push_back(cand);
    *slots[filled++] = cand;
  }
  for (; filled < count && rc == SC_OK; ++filled)
    if (hipStreamCreateWithPriority(slots[filled], hipStreamNonBlocking, 0) != hipSuccess)
      rc = fail(h, SC_ERR_HIP, "could not create a stream for the grouped batch");
  if (sw::group_trace())
    fprintf(stderr, "[sc] streams of the batch: %d on queues of their own, %zu candidates rejected\n",
            (int)have.size(), rejected.size());
  for (hipStream_t r : rejected) (void)hipStreamDestroy(r);
  (void)hipEventDestroy(ea);
  (void)hipEventDestroy(eb);
  return rc;
}

// The member arenas of one bank, before its first front.  Groups of equal cost put a member of
// any size at any position z (five utterances of n ~ 3000 in one batch's first group, seven of
// n ~ 2800 in the next batch's), so every position of a bank that is used at all is reserved for
// the largest member: an arena that has to grow is a hipFree + hipMalloc in the middle of a
// batch (the 8-GPU shares of config 5 ran 3x slower on arenas sized position by position).
int reserve_bank_arenas(sc_handle h, const sc_config* cfg, const EigRequest& rq, int bank,
                        int positions, int largest, int d, const Bands* bands) {
  for (int z = 0; z < positions; ++z) {
    sc_handle hz = nullptr;
    SC_TRY(group_slot(h, bank * kGroupMax + z, &hz));  // (a stride that does not move with the batch)
    int rc = sc_reserve(hz, largest, d);
    // (... and the buffers of the matrix-free Diffuse, which a member arena otherwise grows the
    //  first time a member of n >= 1536 lands in it)
    if (rc == SC_OK && free_diffuse_wanted(hz, cfg, largest, rq, true)) rc = ensure_free(hz, largest);
    if (rc == SC_OK) rc = reserve_constraint(hz, bands, largest);
    if (rc != SC_OK) return fail(h, rc, hz->err);
    hz->have_constraint = false;
  }
  return SC_OK;
}
// The blur weights of the grouped front, resident in the lead before a bank stream reads them.
int upload_group_blur_weights(sc_handle h, const sc_config* cfg) {
  SC_TRY(grow(h, h->blurw, (2 * SC_MAX_BLUR_RADIUS + 1) * sizeof(double)));
  SC_TRY(upload_blur_weights(h, cfg));
  SC_HIP(h, hipStreamSynchronize(h->stream));  // the bank streams read them
  return SC_OK;
}

// One lane of the grouped batch: the groups `mine` (indices into the size-sorted list, `width`
// members each) on the lead's streams and member arenas.
int run_group_lane(sc_handle h, const sc_array* xs, const int* ns, int d,
                   const sc_config* cfg, int64_t* const* labels, sc_diag* diags,
                   const std::vector<int>& grouped, const std::vector<int>& gstart, int width,
                   const std::vector<int>& mine, const EigRequest& rq, int group_limit,
                   const Bands* bands) {
  if (mine.empty()) return SC_OK;
  // (the lead's lockstep chains run on its dedicated stream for the duration of the batch)
  struct StreamSwap {
    sc_handle h;
    hipStream_t saved;
    ~StreamSwap() { h->stream = saved; }
  } swap{h, h->stream};
  SC_HIP(h, hipStreamSynchronize(h->stream));
  h->stream = h->gchain_stream;
  SC_TRY(ensure_seed_table(h));
  memset(h->gconv_hist, 0, sizeof(h->gconv_hist));
  h->gconv_seen = 0;
  const int ngroups = (int)mine.size();
  // Banks of member arenas: while the eigensolver and k-means chains of group g run (short
  // launches, host synchronisations, Rayleigh-Ritz on the host), the GEMMs and refinement
  // passes of group g + 1 keep the chip busy on the other bank's stream.  (Two banks; a
  // third one put two more GEMMs next to the chains and cost 9 % on config 5: the chains'
  // short kernels wait longer for a free CU.)
  constexpr int banks = kGroupBanks;
  // (group g of the size-sorted list = [gstart[g], gstart[g + 1]); `width` = the largest group)
  auto group_count = [&](int j) { return gstart[mine[j] + 1] - gstart[mine[j]]; };
  auto group_members = [&](int j) { return grouped.data() + gstart[mine[j]]; };
  // arenas once (reserve_bank_arenas), every position for the largest member of the lane
  // (the largest grouped member of the BATCH, not of this lane's groups: which lane draws the
  //  large groups changes from batch to batch too)
  const int lane_largest = ns[grouped[0]];
  // (all `group_limit` positions of a bank in use, whatever this batch's largest group: the next
  //  batch -- or the next rank's share -- cuts its list elsewhere, and a position that does not
  //  exist yet is an sc_create: streams, events, pinned buffers, milliseconds)
  for (int b = 0; b < std::min(banks, ngroups); ++b)
    SC_TRY(reserve_bank_arenas(h, cfg, rq, b, std::max(width, group_limit), lane_largest, d, bands));
  Member mbs[kGroupBanks][kGroupMax];
  int front_bank[kGroupBanks];
  const bool trace = sw::group_trace();
  // (a constrained batch never takes the grouped front: its crop value comes out of the affinity
  //  epilogue, which an adjusted affinity invalidates)
  const bool covers = grouped_front_covers(cfg) && !bands;
  if (covers) SC_TRY(upload_group_blur_weights(h, cfg));
  auto front = [&](int j) -> int {
    const int b = j % banks, cnt = group_count(j);
    const int* idx = group_members(j);
    // (the streaming blur of the grouped front needs every member at n >= 256; the sizes
    //  are sorted, the last member of the group is its smallest)
    if (covers && blur_group_front_supported(ns[idx[cnt - 1]], cfg->blur_radius)) {
      front_bank[b] = b;
      return enqueue_front_grouped(h, xs, ns, d, cfg, diags, idx, cnt, b * kGroupMax, mbs[b], b);
    }
    front_bank[b] = -1;
    return enqueue_front(h, xs, ns, d, cfg, diags, idx, cnt, b * kGroupMax, mbs[b], nullptr, bands,
                         h->gbank_stream[b], h->gbank_ev[b]);
  };
  for (int j = 0; j < std::min(banks - 1, ngroups); ++j) SC_TRY(front(j));
  for (int j = 0; j < ngroups; ++j) {
    const double t0 = trace ? now_us() : 0.0;
    if (j + banks - 1 < ngroups) SC_TRY(front(j + banks - 1));
    if (trace) fprintf(stderr, "[sc] next front enqueued in %.0f us\n", now_us() - t0);
    SC_TRY(finish_group(h, ns, cfg, labels, diags, mbs[j % banks], group_count(j), rq,
                        front_bank[j % banks]));
  }
  return SC_OK;
}

// The members of a constrained batch that run as single calls on the caller's handle: each with
// its own band resident for the call (sc_predict with sc_set_constraint_band in front).
int predict_single_banded(sc_handle h, const std::vector<int>& list, const sc_array* xs,
                          const sc_config* cfg, int64_t* const* labels, sc_diag* diags,
                          const Bands& bands) {
  for (int i : list) {
    if (bands.band[i]) SC_TRY(sc_set_constraint_band(h, bands.band[i], (int)xs[i].rows));
    else SC_TRY(sc_clear_constraint(h));
    h->sweep_slot.clear();
    SC_TRY(ingest_embeddings(h, xs[i], xs[i].location == SC_MEM_HOST));
    SC_TRY(sc_run_resident(h, cfg, labels[i], diags ? diags + i : nullptr));
  }
  return sc_clear_constraint(h);
}

// Do the cp[] work matrices of a constrained batch fit?  Worst case: every position of both
// banks of the Lanczos route at the largest grouped member, every position of both wave banks of
// the short route at kDenseMax (what the arenas below reserve); what the arenas already hold counts.
bool constraint_workspace_fits(sc_handle h, const Bands& bands, int largest, bool any_short) {
  if (bands.ncp == 0) return true;
  auto need = [&](const std::vector<sc_handle_s*>& slots, int positions, int n) {
    const size_t nn = (size_t)n * matrix_ld(n) * sizeof(double);
    size_t bytes = 0;
    for (int z = 0; z < positions; ++z)
      for (int i = 0; i < bands.ncp; ++i) {
        const size_t have = z < (int)slots.size() ? slots[z]->cp[i].bytes : 0;
        if (have < nn) bytes += nn;
      }
    return bytes;
  };
  size_t bytes = 0;
  if (largest > 0) bytes += need(h->gslots, kGroupBanks * kGroupMax, largest);
  if (any_short) bytes += need(h->gshort, kGroupBanks * kShortWidth, kDenseMax);
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
  return (double)bytes <= 0.85 * (double)free_b;
}

int predict_batch_core(sc_handle h, const sc_array* xs, const int* ns, int d, int count,
                       const sc_config* cfg, int64_t* const* labels, sc_diag* diags, int group,
                       const Bands& band_set);

}  // namespace

extern "C" int sc_predict_batch_constrained(sc_handle h, const sc_array* xs,
                                            const double* const* bands, int count,
                                            const sc_config* cfg, int64_t* const* labels,
                                            sc_diag* diags, int group) {
  if (!h) return SC_ERR_INVALID;
  if (!xs || !labels || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  if (group < 2)
    return fail(h, SC_ERR_INVALID, "sc_predict_batch_constrained is the grouped form: group >= 2");
  SC_TRY(validate_config(h, cfg));
  SC_HIP(h, hipSetDevice(h->device));
  bool device_source = false;
  std::vector<int> ns(count);
  for (int i = 0; i < count; ++i) {
    SC_TRY(validate_array(h, xs + i));
    if (xs[i].cols != xs[0].cols)
      return fail(h, SC_ERR_INVALID, "all utterances must be (n_i, d) with the same d");
    ns[i] = (int)xs[i].rows;
    device_source |= xs[i].location == SC_MEM_DEVICE;
  }
  SC_TRY(sc_clear_constraint(h));  // the handle's own resident constraint takes no part
  if (count == 0) {
    h->last_routes.clear();
    return SC_OK;
  }
  if (device_source) SC_HIP(h, hipStreamSynchronize(h->stream));  // (as sc_predict_batch_arrays)
  return predict_batch_constrained_impl(h, xs, bands, ns.data(), (int)xs[0].cols, count, cfg,
                                        labels, diags, group);
}

int predict_batch_constrained_impl(sc_handle h, const sc_array* xs, const double* const* bands,
                                   const int* ns, int d, int count, const sc_config* cfg,
                                   int64_t* const* labels, sc_diag* diags, int group) {
  // no band stays resident in a member arena, and none of them is still on its way up from the
  // caller's memory, however the batch ends
  struct Cleanup {
    sc_handle h;
    int rc = SC_OK;
    ~Cleanup() {
      auto clear = [&](const std::vector<sc_handle_s*>& slots) {
        for (sc_handle sub : slots) {
          if (rc != SC_OK) (void)hipStreamSynchronize(sub->stream);
          (void)sc_clear_constraint(sub);
        }
      };
      clear(h->gslots);
      clear(h->gshort);
      for (sc_handle lane : h->glanes) clear(lane->gslots);
      (void)sc_clear_constraint(h);
    }
  } cleanup{h};
  cleanup.rc = predict_batch_core(h, xs, ns, d, count, cfg, labels, diags, group,
                                  make_bands(bands, cfg));
  return cleanup.rc;
}

extern "C" int sc_predict_batch_grouped(sc_handle h, const double* const* xs, const int* ns,
                                        int d, int count, const sc_config* cfg,
                                        int64_t* const* labels, sc_diag* diags, int group) {
  if (!h) return SC_ERR_INVALID;
  if (!xs || !ns || !labels || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  const std::vector<sc_array> arrays = host_f64_arrays(xs, ns, d, count);
  return predict_batch_grouped_impl(h, arrays.data(), ns, d, count, cfg, labels, diags, group);
}

int predict_batch_grouped_impl(sc_handle h, const sc_array* xs, const int* ns, int d, int count,
                               const sc_config* cfg, int64_t* const* labels, sc_diag* diags,
                               int group) {
  return predict_batch_core(h, xs, ns, d, count, cfg, labels, diags, group, Bands());
}

namespace {
// partition, groups, lanes, banks and short waves of a grouped batch; `band_set.band` non-null:
// the constrained batch (one lane, member-by-member fronts, enqueue_front's band handling)
int predict_batch_core(sc_handle h, const sc_array* xs, const int* ns, int d, int count,
                       const sc_config* cfg, int64_t* const* labels, sc_diag* diags, int group,
                       const Bands& band_set) {
  const Bands* bands = band_set.band ? &band_set : nullptr;
  SC_TRY(validate_config(h, cfg));
  SC_HIP(h, hipSetDevice(h->device));
  group = std::max(1, std::min(group, kGroupMax));
  // the batch reuses the member arenas a sweep may have left eigenvectors in
  h->sweep_slot.clear();
  for (sc_handle lane : h->glanes) lane->sweep_slot.clear();
  const EigRequest rq = make_eig_request(cfg);
  const bool cfg_ok = group > 1 && cfg->kmeans_metric == kKmeansCosine &&
                      !constraint_active(h, cfg, true) && !constraint_active(h, cfg, false);
  const bool covered = grouped_front_covers(cfg) && !bands;
  // what ran (sc_last_batch_routes): the routes below report into it while the call runs
  h->last_routes.assign(count, SC_BATCH_ROUTE_SINGLE);
  struct RouteReport {
    sc_handle h;
    ~RouteReport() {
      h->groutes = nullptr;
      for (sc_handle lane : h->glanes) lane->groutes = nullptr;
    }
  } report{h};
  h->groutes = h->last_routes.data();
  std::vector<int> grouped, shorts, single;
  for (int i = 0; i < count; ++i) {
    if (cfg_ok && xs[i].data && ns[i] > 0 && sym_group_eligible(ns[i], rq)) grouped.push_back(i);
    else if (cfg_ok && xs[i].data && ns[i] > 0 && ns[i] <= kDenseMax) shorts.push_back(i);
    else single.push_back(i);
  }
  if (bands) {
    // the chain's work matrices are reserved with the arenas, before the first front: when they
    // do not fit, the members that carry a band run as single calls instead
    int largest = 0;
    bool any_short = false;
    for (int i : grouped) largest = std::max(largest, ns[i]);
    for (int i : shorts) any_short = any_short || bands->band[i];
    if (!constraint_workspace_fits(h, *bands, largest, any_short)) {
      auto hand_over = [&](std::vector<int>& list) {
        std::vector<int> keep;
        for (int i : list) (bands->band[i] ? single : keep).push_back(i);
        list.swap(keep);
      };
      hand_over(grouped);
      hand_over(shorts);
      std::sort(single.begin(), single.end());
    }
  }
  if (!grouped.empty()) {
    // similar sizes together: a group's launches are sized by its largest member
    std::stable_sort(grouped.begin(), grouped.end(), [&](int a, int b) { return ns[a] > ns[b]; });
    // Groups: round 6 -- of equal COST, not equal count.  A group's chains advance in lockstep at
    // the pace of its slowest member and its launches are sized by its largest one; sixteen
    // utterances of n ~ 3000 are 6 ms of work, sixteen of n ~ 400 one.  With equal counts the
    // lane that drew the first group finished long after the others (the 64-utterance share of
    // an 8-GPU run: lanes at 7.4 and 4.2 ms by the cost model).  Now the size-sorted list is cut
    // where the running cost passes total / G (at most `group` members), G a multiple of the lane
    // count with at least two groups per lane (a lane overlaps the front of its next group with
    // the chains of the current one), and the groups go to the lanes longest-first, each to the
    // least loaded lane.  (Round 5's groups of equal count dealt round-robin: the A/B is
    // profiles/r27.)
    auto unit_cost = [&](int i) { const double n = ns[i]; return 60.0 + 3.5e-5 * n * n; };
    std::vector<int> gstart;
    int width = std::min(group, (int)grouped.size());
    const int min_groups = ((int)grouped.size() + width - 1) / width;
    const int lanes_wanted = std::max(
        1, std::min(kGroupLanes, covered ? min_groups / kGroupBanks : 1));
    if (min_groups < 2) {
      for (int at = 0; at < (int)grouped.size(); at += width) gstart.push_back(at);
    } else {
      double total = 0.0;
      for (int i : grouped) total += unit_cost(i);
      const int per_lane = std::max(kGroupBanks, (min_groups + lanes_wanted - 1) / lanes_wanted);
      const int target_groups = lanes_wanted * per_lane;
      const double share = total / target_groups;
      double run = 0.0;
      int start = 0;
      for (int at = 0; at < (int)grouped.size(); ++at) {
        const double c = unit_cost(grouped[at]);
        // close the group before this member if it is full, or if adding the member moves the
        // running cost further from the share than leaving it out
        if (at > start && (at - start >= width || (run + c - share > share - run))) {
          gstart.push_back(start);
          start = at;
          run = 0.0;
        }
        run += c;
      }
      gstart.push_back(start);
    }
    const int ngroups = (int)gstart.size();
    gstart.push_back((int)grouped.size());
    width = 0;
    for (int g = 0; g < ngroups; ++g) width = std::max(width, gstart[g + 1] - gstart[g]);
    // Lanes: the groups of the size-sorted list are dealt round-robin to kGroupLanes leads (the
    // caller's handle and kGroupLanes - 1 more, each with its own streams, member arenas, staging
    // and host workers), and every lead but the first is driven by its own host thread.  The
    // lockstep eigensolver / k-means chain of a group is a string of short launches, host
    // synchronisations and Rayleigh-Ritz solves on the host; with one lane the chains of all
    // groups ran end to end on one stream, and that string -- not the GEMMs -- was the batch's
    // critical path (132 ms of chain against 118 ms of GEMM / refinement kernels on config 5).
    // Measured on config 5 (utterances/s, tests/probes/group_only.py): 1 lane 3800, 2 lanes
    // 4020, 3 lanes 4200, 4 lanes 4150; the second lane's groups in ascending order of size
    // (a GEMM-heavy lane beside a latency-bound one) 3920 against 4020.
    const int lanes =
        std::max(1, std::min(kGroupLanes, covered ? ngroups / kGroupBanks : 1));
    std::vector<int> lane_groups[kGroupLanes];
    {  // longest group first, each to the least loaded lane (ties: the lower lane)
      std::vector<double> gcost(ngroups, 0.0);
      for (int g = 0; g < ngroups; ++g)
        for (int at = gstart[g]; at < gstart[g + 1]; ++at) gcost[g] += unit_cost(grouped[at]);
      std::vector<int> order(ngroups);
      for (int g = 0; g < ngroups; ++g) order[g] = g;
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return gcost[a] > gcost[b]; });
      double load[kGroupLanes] = {0.0};
      for (int g : order) {
        int best = 0;
        for (int l = 1; l < lanes; ++l)
          if (load[l] < load[best]) best = l;
        lane_groups[best].push_back(g);
        load[best] += gcost[g];
      }
    }
    sc_handle leads[kGroupLanes] = {h};
    for (int l = 1; l < lanes; ++l) {
      while ((int)h->glanes.size() < l) {
        sc_handle lane = nullptr;
        const int rc = sc_create(h->device, &lane);
        if (rc != SC_OK) return fail(h, rc, "could not create a lane of the grouped batch");
        lane->profile_level = 1;
        h->glanes.push_back(lane);
      }
      leads[l] = h->glanes[l - 1];
      leads[l]->blur_ext = h->blur_ext;
      leads[l]->err.clear();
      leads[l]->groutes = h->groutes;
    }
    // The streams of the batch: per lane one for the lockstep chains and one per bank for the
    // fronts, on hardware queues of their own (independent_streams above); the leads' own streams
    // idle during the batch.
    {
      hipStream_t* want[kGroupLanes * (1 + kGroupBanks)];
      int nwant = 0;
      for (int pass = 0; pass < 1 + kGroupBanks; ++pass)  // (the chains first: they matter most)
        for (int l = 0; l < lanes; ++l) {
          hipStream_t* slot =
              pass == 0 ? &leads[l]->gchain_stream : &leads[l]->gbank_stream[pass - 1];
          if (!*slot) want[nwant++] = slot;
          if (pass > 0 && !leads[l]->gbank_ev[pass - 1])
            SC_HIP(h, hipEventCreateWithFlags(&leads[l]->gbank_ev[pass - 1], hipEventDisableTiming));
        }
      if (nwant > 0) {
        std::vector<hipStream_t> have;  // (lanes of an earlier, smaller batch keep theirs)
        for (int l = 0; l < lanes; ++l) {
          if (leads[l]->gchain_stream) have.push_back(leads[l]->gchain_stream);
          for (int b2 = 0; b2 < kGroupBanks; ++b2)
            if (leads[l]->gbank_stream[b2]) have.push_back(leads[l]->gbank_stream[b2]);
        }
        SC_TRY(independent_streams(h, have, want, nwant));
      }
    }
    int rcs[kGroupLanes] = {SC_OK};
    std::vector<std::thread> side;
    bool inline_lane[kGroupLanes] = {false};
    for (int l = 1; l < lanes; ++l) {
      auto body = [&, l]() {
        if (hipSetDevice(h->device) != hipSuccess) {
          rcs[l] = fail(leads[l], SC_ERR_HIP, "hipSetDevice failed on a lane");
          return;
        }
        rcs[l] = run_group_lane(leads[l], xs, ns, d, cfg, labels, diags, grouped, gstart, width,
                                lane_groups[l], rq, group, bands);
      };
      try {
        side.emplace_back(body);
      } catch (...) {  // (no thread to be had: the lane runs on this one, after lane 0)
        inline_lane[l] = true;
      }
    }
    rcs[0] = run_group_lane(h, xs, ns, d, cfg, labels, diags, grouped, gstart, width,
                            lane_groups[0], rq, group, bands);
    for (int l = 1; l < lanes; ++l)
      if (inline_lane[l])
        rcs[l] = run_group_lane(leads[l], xs, ns, d, cfg, labels, diags, grouped, gstart, width,
                                lane_groups[l], rq, group, bands);
    for (auto& t : side) t.join();
    {  // member arenas that hold a large share of the device do not outlive the batch (the
       // lanes keep up to 3 x 2 x 16 of them warm otherwise: 21 GB after config 5)
      size_t free_b = 0, total_b = 0, held = 0;
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        for (int l = 0; l < lanes; ++l)
          for (sc_handle sub : leads[l]->gslots) {
            held += sub->A0.bytes + sub->B1.bytes + sub->B2.bytes;
            for (const DevBuf& w : sub->cp) held += w.bytes;  // (a constrained batch's work matrices)
          }
        if (held > total_b / 4)
          for (int l = 0; l < lanes; ++l) {
            for (sc_handle sub : leads[l]->gslots) sc_destroy(sub);
            leads[l]->gslots.clear();
            leads[l]->sweep_slot.clear();
          }
      }
    }
    if (rcs[0] != SC_OK) return rcs[0];
    for (int l = 1; l < lanes; ++l)
      if (rcs[l] != SC_OK) return fail(h, rcs[l], leads[l]->err.c_str());
  }
  // the short route (n <= kDenseMax), once the lanes of the Lanczos route are done: waves of
  // kShortWidth members, largest first (a wave's Jacobi launch lasts as long as its largest member)
  if (!shorts.empty()) {
    std::stable_sort(shorts.begin(), shorts.end(), [&](int a, int b) { return ns[a] > ns[b]; });
    SC_TRY(run_short_route(h, xs, ns, d, cfg, labels, diags, shorts, rq, bands));
  }
  // (members outside the grouped path's range -- n >= 4096 above all: their uploads ride under
  //  the previous member's pipeline, api.hip predict_sequence)
  if (!single.empty() && bands)
    SC_TRY(predict_single_banded(h, single, xs, cfg, labels, diags, *bands));
  else if (!single.empty())
    SC_TRY(predict_sequence(h, single.data(), (int)single.size(), xs, ns, d, cfg, labels, diags));
  return SC_OK;
}
}  // namespace

namespace {
// What sc_eig_ncluster_sweep decides before its rounds: which of the two sequences it groups,
// whether the level runs as a group at all, and the route of its Diffuse.
struct SweepPlan {
  bool icassp = false, thr_sym_only = false, grouped = false;
  bool free_route = false, amax_from_cut = false;
  // n <= kDenseMax: the level's values as (matrix, p) pairs -- one front launch and ONE Jacobi
  // launch for up to kShortWidth of them (sweep_short_level)
  bool short_level = false;
};
SweepPlan sweep_plan(sc_handle h, const sc_config* cfg, int count, const EigRequest& rq) {
  const int n = h->n;
  SweepPlan plan;
  // Two sequences are swept as groups: the ICASSP2018 one, and [RowWiseThreshold, Symmetrize]
  // alone -- the Turn-to-Diarize refinement (reference configs.py:49-59: Percentile cut,
  // binarisation, preserved diagonal, Average), whose values are the thresholded affinity
  // itself: no blur to share, no Diffuse, the lockstep solver works on the symmetrised matrix.
  plan.icassp = grouped_front_covers(cfg);
  plan.thr_sym_only = cfg->n_ops == 2 && cfg->ops[0] == SC_OP_ROW_WISE_THRESHOLD &&
                      cfg->ops[1] == SC_OP_SYMMETRIZE;
  plan.grouped = count > 1 && (plan.icassp || plan.thr_sym_only) && h->affinity_symmetric &&
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
  plan.short_level = !plan.grouped && count > 1 && n <= kDenseMax &&
                     (plan.icassp || plan.thr_sym_only) && h->affinity_symmetric &&
                     !constraint_active(h, cfg, false) && !plan.free_route &&
                     !sw::sweep_one_by_one();
  return plan;
}

// The part of the ICASSP2018 front every value of a level shares: CropDiagonal's value and the
// blurred matrix (+ per-strip row maxima) of the resident affinity, on the handle's stream.
// `crop` (may be null): where the value vector the blur read lies; `crop_source`: as FrontResult's.
int sweep_shared_blur(sc_handle h, const sc_config* cfg, const double** crop_out = nullptr,
                      int* crop_source = nullptr) {
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
                        int slot0 = 0, sc_handle owner = nullptr) {
  *out_of_memory = false;
  const int n = h->n, ld = h->ldn;
  const bool icassp = plan.icassp, free_route = plan.free_route;
  const int nt = gemm_tile_dim(n);
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
    FrontItem& f = fi[z];
    f.n = n;
    f.ldn = ld;
    // the matrix every value thresholds: the shared blurred one, or the affinity itself
    f.B1 = icassp ? ptr<double>(h->B1) : ptr<double>(h->A0);  // read only
    f.B2 = ptr<double>(hz->B2);
    f.rmpart = ptr<double>(h->rmpart);
    f.blur_cols = blur_tile_columns(n, cfg->blur_radius);
    f.cut = ptr<double>(hz->cut);
    f.rowmax = ptr<double>(hz->rowmax);
    f.rowsum = ptr<double>(hz->rowsum);
    f.cvec = ptr<double>(hz->cvec);
    f.pvec = ptr<double>(hz->pvec);
    f.tvec = ptr<double>(hz->tvec);
    f.symflag = h->affinity_from_embeddings ? ptr<int>(h->symflag) : nullptr;
    f.flags = ptr<int>(hz->flags);
    f.p_own = ps[z];
    dif[z] = GemmGroupItem();
    dif[z].A = f.B2;
    dif[z].lda = ld;
    dif[z].C = ptr<double>(hz->B1);
    dif[z].ldc = ld;
    dif[z].n = n;
    dif[z].K = n;
    dif[z].tilemap = hz->tilemap_cur;
    dif[z].partial_max = ptr<double>(hz->statp);
    dif[z].partial_sum = ptr<double>(hz->statp) + (size_t)n * nt;
    dif[z].rowmax = ptr<double>(hz->rowmax);
    dif[z].rowsum = ptr<double>(hz->rowsum);
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
                      FrontResult* taken = nullptr) {
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
struct ShortShared {
  const double* src = nullptr;   // the matrix every value thresholds
  const double* crop = nullptr;  // CropDiagonal's value vector (fused form only)
  int crop_source = 0;
};
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
      sc_diag* dg = diags + base + z;
      memset(dg, 0, sizeof(*dg));
      dg->n = n;
      dg->n_clusters_raw = em[z].dc.n_clusters_raw;
      dg->max_delta = em[z].dc.max_delta;
      dg->eig_descending = rq.descend;
      dg->n_eigenvalues = std::min((int)em[z].w.size(), SC_MAX_EIG);
      for (int i = 0; i < dg->n_eigenvalues; ++i) dg->eigenvalues[i] = em[z].w[i];
      dg->symmetry_state = plan.icassp ? 2 : 1;
      dg->eig_path = SC_EIG_PATH_DENSE_JACOBI;
      dg->diffuse_path = plan.icassp ? SC_DIFFUSE_PATH_EXPLICIT : SC_DIFFUSE_PATH_NONE;
    }
  }
  *handled = true;
  for (int i : later) {  // (the single call states the error, or finds what the group did not)
    sc_config c = *cfg;
    c.p_percentile = p_values[i];
    SC_TRY(sc_eig_ncluster(h, &c, diags + i));
  }
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
  auto one_by_one = [&](int i) -> int {
    sc_config c = *cfg;
    c.p_percentile = p_values[i];
    return sc_eig_ncluster(h, &c, diags + i);
  };
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
      sc_diag* dg = diags + base + z;
      if (em[z].status == 0) h->sweep_slot[base + z] = z;
      if (em[z].status != 0) {
        later.push_back(base + z);  // (after the rounds: it overwrites the shared blur)
        continue;
      }
      memset(dg, 0, sizeof(*dg));
      dg->n = n;
      dg->n_clusters_raw = em[z].dc.n_clusters_raw;
      dg->max_delta = em[z].dc.max_delta;
      dg->eig_descending = rq.descend;
      dg->n_eigenvalues = std::min((int)em[z].w.size(), SC_MAX_EIG);
      for (int i = 0; i < dg->n_eigenvalues; ++i) dg->eigenvalues[i] = em[z].w[i];
      dg->symmetry_state = icassp ? 2 : 1;
      dg->eig_path = SC_EIG_PATH_BLOCK_LANCZOS;
      dg->eig_matvec_passes = em[z].passes;
      dg->eig_block = kEigBlock;
      dg->eig_basis = em[z].basis;
      dg->eig_max_residual = em[z].dc.max_resid;
      dg->diffuse_path = !icassp ? SC_DIFFUSE_PATH_NONE
                                 : (free_route ? SC_DIFFUSE_PATH_FREE : SC_DIFFUSE_PATH_EXPLICIT);
      if (free_route) {
        dg->free_candidates = em[z].h->h_free[65];
        dg->free_tiles_run = em[z].h->h_free[67];
      }
    }
  }
  SC_HIP(h, hipStreamSynchronize(s));
  {  // member arenas that hold a large share of the device do not outlive the sweep
    size_t free_b = 0, total_b = 0, held = 0;
    SC_HIP(h, hipMemGetInfo(&free_b, &total_b));
    for (sc_handle sub : h->gslots) held += sub->A0.bytes + sub->B1.bytes + sub->B2.bytes;
    if (out_of_memory || held > total_b / 4) {
      for (sc_handle sub : h->gslots) sc_destroy(sub);
      h->gslots.clear();
      h->sweep_slot.assign(count, -1);
    }
  }
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


// ------------------------------------------------------------------------------
// sc_stage_front: what the fused refinement front leaves behind (tests)
// ------------------------------------------------------------------------------
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
  FrontWhere w;
  w.h = h;
  w.n = n;
  w.ld = h->ldn;
  w.a0 = ptr<double>(h->A0);
  w.cropval = fr.crop_source == 1 ? ptr<double>(h->cropval)
                                  : (fr.crop_source == 2 ? ptr<double>(h->dvec) : nullptr);
  w.cut = fr.cut_kernel != 0 ? ptr<double>(h->cut) : nullptr;
  // (the explicit product wrote S into the buffer after A's: `scratch` is still A)
  w.a = fr.diffuse_explicit ? fr.scratch : fr.matrix;
  w.s = fr.diffuse_explicit ? fr.matrix : nullptr;
  w.diffuse_path = fr.free_op ? SC_DIFFUSE_PATH_FREE
                              : (fr.diffuse_explicit ? SC_DIFFUSE_PATH_EXPLICIT
                                                     : SC_DIFFUSE_PATH_NONE);
  w.symmetric = fr.symmetric;
  w.folded_rownorm = fr.folded_rownorm;
  w.free_op = fr.free_op;
  w.digits_fused = fr.digits_fused;
  w.blur = h->last_blur;
  w.crop_source = fr.crop_source;
  w.cut_kernel = fr.cut_kernel;
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
  for (int z = 0; z < count; ++z) {
    sc_handle hz = mb[z].h;
    const FrontResult& fr = mb[z].front;
    FrontWhere w;
    w.h = hz;
    w.n = ns[z];
    w.ld = hz->ldn;
    w.a0 = ptr<double>(hz->A0);
    w.cropval = ptr<double>(hz->cropval);
    w.cut = ptr<double>(hz->cut);
    w.a = ptr<double>(hz->B2);
    w.s = fr.diffuse_explicit ? ptr<double>(hz->B1) : nullptr;
    w.diffuse_path = fr.free_op ? SC_DIFFUSE_PATH_FREE
                                : (fr.diffuse_explicit ? SC_DIFFUSE_PATH_EXPLICIT
                                                       : SC_DIFFUSE_PATH_NONE);
    w.symmetric = fr.symmetric;
    w.folded_rownorm = fr.folded_rownorm;
    w.free_op = fr.free_op;
    w.digits_fused = fr.digits_fused;
    w.blur = h->last_blur;
    w.crop_source = fr.crop_source;
    w.cut_kernel = fr.cut_kernel;
    SC_TRY(front_copy_out(h, w, outs + z));
  }
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
    sc_handle hz = em[z].h;
    FrontWhere w;
    w.h = hz;
    w.n = n;
    w.ld = h->ldn;
    w.a0 = ptr<double>(h->A0);
    w.cropval = crop;
    w.cut = taken[z].cut_kernel != 0 ? ptr<double>(hz->cut) : nullptr;
    w.a = ptr<double>(hz->B2);
    w.s = taken[z].diffuse_explicit ? ptr<double>(hz->B1) : nullptr;
    w.diffuse_path = em[z].free_op ? SC_DIFFUSE_PATH_FREE
                                   : (taken[z].diffuse_explicit ? SC_DIFFUSE_PATH_EXPLICIT
                                                                : SC_DIFFUSE_PATH_NONE);
    w.folded_rownorm = plan.icassp;  // (launch_scaling_vectors_group's row_normalized)
    w.free_op = em[z].free_op;
    w.digits_fused = taken[z].digits_fused;
    w.blur = h->last_blur;
    w.crop_source = crop_source;
    w.cut_kernel = taken[z].cut_kernel;
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
    sc_handle hz = em[z].h;
    FrontWhere w;
    w.h = hz;
    w.n = n;
    w.ld = h->ldn;
    w.a0 = ptr<double>(h->A0);
    w.cropval = sh.crop;
    w.cut = ptr<double>(hz->cut);
    w.a = ptr<double>(hz->B2);
    w.s = plan.icassp ? ptr<double>(hz->B1) : nullptr;
    w.diffuse_path = plan.icassp ? SC_DIFFUSE_PATH_EXPLICIT : SC_DIFFUSE_PATH_NONE;
    w.folded_rownorm = plan.icassp;
    w.blur = h->last_blur;
    w.crop_source = sh.crop_source;
    w.cut_kernel = 4;
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
    sc_handle hz = mb[z].h;
    const FrontResult& fr = mb[z].front;
    FrontWhere w;
    w.h = hz;
    w.n = ns[z];
    w.ld = hz->ldn;
    w.a0 = ptr<double>(hz->A0);
    // (the vector is reported where a single call reports one: its fused crop + blur, which it
    //  takes from n = 128 on at radius 4 or 8 -- below, its CropDiagonal leaves a matrix only)
    const bool single_reports = ops.crop && (ops.blur_radius == 4 || ops.blur_radius == 8) &&
                                ns[z] >= 128;
    w.cropval = single_reports ? ptr<double>(hz->cropval) : nullptr;
    w.cut = ptr<double>(hz->cut);
    w.a = ptr<double>(hz->B2);
    w.s = fr.diffuse_explicit ? ptr<double>(hz->B1) : nullptr;
    w.diffuse_path = fr.diffuse_explicit ? SC_DIFFUSE_PATH_EXPLICIT : SC_DIFFUSE_PATH_NONE;
    w.symmetric = fr.symmetric;
    w.folded_rownorm = fr.folded_rownorm;
    w.crop_source = single_reports ? fr.crop_source : 0;
    w.cut_kernel = fr.cut_kernel;
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

// ------------------------------------------------------------------------------
// sc_predict_batch_autotune: a batch in which every utterance is an AutoTune search
// ------------------------------------------------------------------------------
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
  std::vector<int> ns(count);
  for (int i = 0; i < count; ++i) {  // every descriptor before the first launch
    SC_TRY(validate_array(h, xs + i));
    if (!labels[i]) return fail(h, SC_ERR_INVALID, "NULL labels");
    if (xs[i].cols != xs[0].cols)
      return fail(h, SC_ERR_INVALID, "all utterances must be (n_i, d) with the same d");
    ns[i] = (int)xs[i].rows;
    device_source |= xs[i].location == SC_MEM_DEVICE;
  }
  SC_TRY(sc_clear_constraint(h));  // the handle's own resident constraint takes no part
  h->last_routes.assign(count, SC_BATCH_ROUTE_SINGLE);
  if (count == 0) return SC_OK;
  if (device_source) SC_HIP(h, hipStreamSynchronize(h->stream));  // (as sc_predict_batch_arrays)
  const int d = (int)xs[0].cols;
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
  SweepPlan probe;  // (which sequences the sweep groups: the configuration alone decides)
  probe.icassp = grouped_front_covers(cfg);
  probe.thr_sym_only = cfg->n_ops == 2 && cfg->ops[0] == SC_OP_ROW_WISE_THRESHOLD &&
                       cfg->ops[1] == SC_OP_SYMMETRIZE;
  const bool swept = (probe.icassp || probe.thr_sym_only) && cfg->kmeans_metric == kKmeansCosine &&
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
  {
    double load[kGroupLanes] = {0.0};
    for (int i : mids) {
      int best = 0;
      for (int l = 1; l < lanes; ++l)
        if (load[l] < load[best]) best = l;
      lane_list[best].push_back(i);
      load[best] += 60.0 + 3.5e-5 * (double)ns[i] * ns[i];
    }
  }
  sc_handle leads[kGroupLanes] = {h};
  for (int l = 1; l < lanes; ++l) {
    while ((int)h->glanes.size() < l) {
      sc_handle lane = nullptr;
      const int rc = sc_create(h->device, &lane);
      if (rc != SC_OK) return cleanup.rc = fail(h, rc, "could not create a lane of the AutoTune batch");
      lane->profile_level = 1;
      h->glanes.push_back(lane);
    }
    leads[l] = h->glanes[l - 1];
    leads[l]->blur_ext = h->blur_ext;
    leads[l]->err.clear();
  }
  int32_t* routes = h->last_routes.data();
  auto run_lane = [&](int l) -> int {
    sc_handle lead = leads[l];
    if (hipSetDevice(lead->device) != hipSuccess) return SC_ERR_HIP;
    for (int i : lane_list[l]) {
      const int rc = autotune_one(lead, xs[i], bands ? bands[i] : nullptr, cfg, at, labels[i],
                                  diags ? diags + i : nullptr, best_p ? best_p + i : nullptr,
                                  last_p ? last_p + i : nullptr);
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
    const int i = single[q];
    rc = autotune_one(h, xs[i], bands ? bands[i] : nullptr, cfg, at, labels[i],
                      diags ? diags + i : nullptr, best_p ? best_p + i : nullptr,
                      last_p ? last_p + i : nullptr);
    routes[i] = SC_BATCH_ROUTE_SINGLE;
  }
  return cleanup.rc = rc;
}
