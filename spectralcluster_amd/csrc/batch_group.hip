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
// (enqueue_front; constraint_api.hip: constraint_propagation_group).  A member's constraint may
// also be an entry list or a dense matrix given as a described source
// (sc_predict_batch_constraint_arrays): the dense sources of a front are widened into the member
// arenas' Cq by the grouped ingest, together with the affinities where the batch's arrays are those.
#include <ctime>
#include <thread>
#include <utility>

#include "batch_internal.h"

namespace {

double now_us() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}

// The Bands of a constrained batch under `cfg` ...
Bands make_bands(const sc_constraint_desc* cons, const std::vector<double>* packed,
                 const char* pairs_symmetric, int kmax, const sc_config* cfg,
                 const sc_array* dense) {
  Bands b;
  if (cfg->constraint_name == SC_CONSTRAINT_NONE) return b;  // (nothing would read them)
  b.cons = cons;
  b.dense = dense;
  b.packed = packed;
  b.pairs_symmetric = pairs_symmetric;
  b.kmax = kmax;
  if (cfg->constraint_name == SC_CONSTRAINT_PROPAGATION) {
    b.chain = cfg->constraint_before_refinement != 0;
    // the grouped chain works in B1 / B2 (idle until refinement starts) + two more matrices; after
    // refinement the member's own constraint_propagation() takes its five
    b.ncp = b.chain ? 2 : 5;
  }
  return b;
}
// ... and what a member arena holds for it, reserved with the arena (never inside a front).  The
// one exception is the staging of a front's HOST dense sources (and host affinities), which lies
// in the first arena's Xstage at the sources' own width and grows in the first front that needs
// more (ingest_member_sources); constraint_workspace_fits counts its worst case.
int reserve_constraint(sc_handle hz, const Bands* bands, int n_max) {
  if (!bands || (!bands->cons && !bands->dense)) return SC_OK;
  // (a dense member's matrix: the ingest kernel widens its source into Cq)
  if (bands->dense)
    SC_TRY(grow(hz, hz->Cq, (size_t)n_max * matrix_ld(n_max) * sizeof(double)));
  SC_TRY(grow(hz, hz->Cband, (size_t)std::max(n_max - 1, 1) * sizeof(double)));
  if (bands->kmax > 0) {  // entries (16 bytes each) and AffinityIntegration's gathered originals
    SC_TRY(grow(hz, hz->Cpairs, (size_t)bands->kmax * 2 * sizeof(double)));
    SC_TRY(grow(hz, hz->Cporig, (size_t)bands->kmax * sizeof(double)));
  }
  const size_t nn = (size_t)n_max * matrix_ld(n_max) * sizeof(double);
  for (int i = 0; i < bands->ncp; ++i) SC_TRY(grow(hz, hz->cp[i], nn));
  return SC_OK;
}

// Arena `h` now holds a member's problem: its rows go in on stream `s`, ahead of the front's
// launches (arena and problem size are set by the same call), and its state is that of an affinity
// computed from embeddings.  have_cropval and the resident constraint are the calling front's.
int member_problem(sc_handle lead, sc_handle h, const sc_array& x, int n, int d, hipStream_t s) {
  h->err.clear();
  int rc = ingest_embeddings(h, x, false, s);
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
  h->affinity_symmetric = h->affinity_from_embeddings = true;
  h->constraint_applied = false;
  return SC_OK;
}

// The members of a front whose arrays are the callers' affinities (Bands::affinities) and the dense
// constraints its members carry (Bands::dense): grouped ingest launches on `s`, one per 64
// sources, widen every affinity into its arena's A0 and every dense constraint into its arena's Cq
// and leave the sources' symmetry flags in one device array, which the host reads once -- the
// front's only wait; the arenas of ingested affinities then are in the state sc_set_affinity_array
// leaves, and dense_symmetric[z] says what member z's constraint is (enqueue_front makes it the
// arena's resident constraint).  Descriptor table, flags and the staging rows of host members live
// in the first arena's staging buffer (the group owns it).
int ingest_member_sources(sc_handle lead, const sc_array* xs, const int* idx, int count,
                          int slot0, std::vector<sc_handle_s*>* arenas, hipStream_t s,
                          const Bands& bands, std::vector<char>* dense_symmetric) {
  std::vector<sc_array> as;
  std::vector<double*> dsts;
  std::vector<sc_handle> hs(count);
  std::vector<int> dense_at(count, -1);
  dense_symmetric->assign(count, 0);
  for (int z = 0; z < count; ++z) {
    SC_TRY(group_slot(lead, slot0 + z, &hs[z], arenas));
    sc_handle h = hs[z];
    h->err.clear();
    const int n = (int)xs[idx[z]].rows;
    int rc = SC_OK;
    if (bands.affinities) {
      rc = ensure_matrices(h, n, 0);
      if (rc == SC_OK) rc = ensure_tilemap(h, n);
      if (rc == SC_OK) rc = grow(h, h->symflag, 16);
    }
    if (rc != SC_OK) return fail(lead, rc, h->err);
    if (bands.affinities) {
      as.push_back(xs[idx[z]]);
      dsts.push_back(ptr<double>(h->A0));
    }
  }
  for (int z = 0; z < count; ++z) {  // (behind the affinities: flags[z] stays member z's affinity)
    if (!bands.is_dense(idx[z])) continue;
    sc_handle h = hs[z];
    const int n = (int)bands.dense[idx[z]].rows;
    // (reserved with the arena: reserve_constraint)
    if (grow(h, h->Cq, (size_t)n * matrix_ld(n) * sizeof(double)) != SC_OK)
      return fail(lead, SC_ERR_OOM, h->err);
    dense_at[z] = (int)as.size();
    as.push_back(bands.dense[idx[z]]);
    dsts.push_back(ptr<double>(h->Cq));
  }
  const int total = (int)as.size();
  if (total == 0) return SC_OK;
  std::vector<int> flags(total, 0);
  auto align256 = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t table_at = align256(total * sizeof(int));
  const size_t stage_at = table_at + align256(total * affinity_group_table_bytes());
  sc_handle h0 = hs[0];
  if (grow(h0, h0->Xstage, stage_at + affinity_group_stage_bytes(as.data(), total)) != SC_OK)
    return fail(lead, SC_ERR_OOM, h0->err);
  unsigned char* base = static_cast<unsigned char*>(h0->Xstage.p);
  SC_TRY(ingest_affinity_group(lead, as.data(), total, dsts.data(), reinterpret_cast<int*>(base),
                               base + stage_at, base + table_at, s, flags.data()));
  for (int z = 0; z < count; ++z) {
    if (dense_at[z] >= 0) (*dense_symmetric)[z] = flags[dense_at[z]] != 0 ? 1 : 0;
    if (!bands.affinities) continue;
    sc_handle h = hs[z];
    h->n = (int)xs[idx[z]].rows;
    h->d = 0;
    h->ldn = matrix_ld(h->n);
    h->ldx = 0;
    h->n_vec = 0;
    h->have_x = h->have_cropval = false;
    h->have_affinity = true;
    h->affinity_symmetric = flags[z] != 0;
    h->affinity_from_embeddings = false;
    h->constraint_applied = false;
  }
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
  const bool affinities = bands && bands->affinities;
  std::vector<char> dense_symmetric;  // of the members that carry a dense constraint
  if (affinities || (bands && bands->dense))
    SC_TRY(ingest_member_sources(lead, xs, idx, count, slot0, arenas, chain_stream, *bands,
                                 &dense_symmetric));
  for (int z = 0; z < count; ++z) {
    Member& m = mb[z];
    m = Member();
    m.index = idx[z];
    SC_TRY(group_slot(lead, slot0 + z, &m.h, arenas));
    sc_handle h = m.h;
    h->err.clear();
    // (no wait: the caller's arrays stay valid for the whole batch call)
    int rc = affinities ? SC_OK : ingest_embeddings(h, xs[m.index], false);
    h->nev = 0;
    if (diags) memset(diags + m.index, 0, sizeof(sc_diag));
    if (rc == SC_OK && !affinities) rc = sc_compute_affinity(h);
    // the arena's resident constraint is this member's band or entry list, or none
    h->have_constraint = h->constraint_banded = h->constraint_pairs = false;
    h->qn = 0;
    const double* band = bands ? bands->band(m.index) : nullptr;
    const bool pairs = bands && bands->pairs(m.index);
    if (rc == SC_OK && pairs) {
      // (buffers reserved with the arena for the batch's largest list: reserve_constraint)
      const int k = bands->cons[m.index].count;
      const size_t bytes = (size_t)k * 2 * sizeof(double);
      if (h->Cpairs.bytes < bytes || h->Cporig.bytes < (size_t)k * sizeof(double))
        rc = fail(h, SC_ERR_INVALID, "member arena without the entry buffers");
      if (rc == SC_OK && bytes > 0 &&
          hipMemcpyAsync(h->Cpairs.p, bands->packed[m.index].data(), bytes, hipMemcpyHostToDevice,
                         h->stream) != hipSuccess)
        rc = fail(h, SC_ERR_HIP, "could not upload a constraint entry list");
      h->have_constraint = h->constraint_pairs = true;
      h->constraint_symmetric = bands->pairs_symmetric[m.index] != 0;
      h->pairs_count = k;
      h->qn = h->n;
    }
    // (the grouped chain works on symmetric affinities: a caller's matrix that is not symmetric
    //  takes the member's own operator below)
    const bool chain = bands && bands->chain && h->affinity_symmetric;
    if (rc == SC_OK && bands && bands->is_dense(m.index)) {
      // (its matrix is in Cq already: ingest_member_sources)
      h->have_constraint = true;
      h->constraint_symmetric = dense_symmetric[z] != 0;
      h->qn = h->n;
      // (the chain's dense stage is the symmetric one; any other Q takes the member's own operator)
      if (chain && h->constraint_symmetric) {
        chained.push_back(z);
        SC_HIP(lead, hipEventRecord(h->sync_ev, h->stream));  // "the affinity is there"
        continue;
      }
    }
    if (rc == SC_OK && pairs && chain) {
      chained.push_back(z);
      SC_HIP(lead, hipEventRecord(h->sync_ev, h->stream));  // "affinity and entries are there"
      continue;
    }
    if (rc == SC_OK && band) {
      const size_t bytes = (size_t)(h->n - 1) * sizeof(double);
      rc = grow(h, h->Cband, std::max<size_t>(bytes, sizeof(double)));
      if (rc == SC_OK && bytes > 0 &&
          hipMemcpyAsync(h->Cband.p, band, bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess)
        rc = fail(h, SC_ERR_HIP, "could not upload a constraint band");
      h->have_constraint = h->constraint_banded = h->constraint_symmetric = true;
      h->qn = h->n;
    }
    if (rc == SC_OK && band && chain) {
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
      if (h->constraint_pairs) {
        cm[q].pairs = true;
        cm[q].psym = h->constraint_symmetric;
        cm[q].pk = h->pairs_count;
        cm[q].pvals = ptr<double>(h->Cpairs);
        cm[q].prows = reinterpret_cast<const int32_t*>(cm[q].pvals + cm[q].pk);
        cm[q].pcols = cm[q].prows + cm[q].pk;
      } else if (!h->constraint_banded) {  // a dense symmetric matrix
        if (h->Cq.bytes < nn)
          return fail(lead, SC_ERR_INVALID, "member arena without the dense constraint matrix");
        cm[q].q = ptr<double>(h->Cq);
      }
    }
    SC_TRY(constraint_propagation_group(lead, chain_stream, cm, cnt, cfg->constraint_alpha));
  }
  SC_HIP(lead, hipEventRecord(chain_ev, chain_stream));
  for (int z : chained) {
    sc_handle h = mb[z].h;
    SC_HIP(lead, hipStreamWaitEvent(h->stream, chain_ev, 0));
    h->have_cropval = false;  // (what sc_apply_constraint leaves: the epilogue's crop values are stale)
    h->affinity_symmetric = h->affinity_symmetric && h->constraint_symmetric;  // (a band is)
    h->constraint_applied = true;
    h->n_vec = 0;
    SC_TRY(refine(z));
  }
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

// The hand-over of a front: the owner's stream waits for the bank's event (`front_bank` >= 0:
// grouped launches on that bank's stream) or for every member's own; the members still in the
// group (state 0) are collected for the lockstep solver, *ne of them: em[e] is member emz[e].
int take_front(sc_handle lead, const int* ns, Member* mb, int count, const EigRequest& rq,
               int front_bank, GroupEigMember* em, int* emz, int* ne) {
  hipStream_t s = lead->stream;
  if (front_bank >= 0) {
    SC_HIP(lead, hipStreamWaitEvent(s, lead->gbank_ev[front_bank], 0));
  } else {
    for (int z = 0; z < count; ++z) SC_HIP(lead, hipStreamWaitEvent(s, mb[z].h->sync_ev, 0));
  }
  *ne = 0;
  for (int z = 0; z < count; ++z) {
    if (mb[z].state != 0) continue;  // (a front that is not symmetric: the general solver)
    GroupEigMember& g = em[*ne];
    g = GroupEigMember();
    g.h = mb[z].h;
    g.S = mb[z].front.matrix;
    g.ld = mb[z].front.ld;
    g.n = ns[mb[z].index];
    g.rq = rq;
    g.free_op = mb[z].front.free_op;  // (the dense solve of the short route does not read it)
    mb[z].eig = &g;
    emz[(*ne)++] = z;
  }
  return SC_OK;
}

// min_clusters = 1: the single-cluster test of a group's (`wave`: a short wave's) members on their
// raw affinities, as group-wide device work on the owner's stream behind the front's hand-over
// (single_check.hip).  A0 is read only: no front of an unconstrained batch writes it after the
// affinity product.  The front of the next group or wave is already enqueued on the other bank's
// stream, so the chip works on it while the host waits for the members' state.  A member found to
// hold one cluster leaves here -- state 2, labels of zeros, a zeroed diag; its refinement front
// ran speculatively -- and never enters the eigensolver.
int decide_single(sc_handle lead, const int* ns, int64_t* const* labels, sc_diag* diags,
                  Member* mb, int count, int front_bank, bool wave, int route,
                  const SingleCheck* sc) {
  if (!sc || count <= 0) return SC_OK;
  hipStream_t s = lead->stream;
  if (front_bank >= 0) {
    SC_HIP(lead, hipStreamWaitEvent(s, lead->gbank_ev[front_bank], 0));
  } else {
    for (int z = 0; z < count; ++z) SC_HIP(lead, hipStreamWaitEvent(s, mb[z].h->sync_ev, 0));
  }
  std::vector<SingleMember> ms(count);
  std::vector<int32_t> one(count, 0);
  for (int z = 0; z < count; ++z)
    ms[z] = SingleMember{ptr<double>(mb[z].h->A0), mb[z].h->n, mb[z].h->ldn};
  SC_TRY(wave ? single_check_wave(lead, s, ms.data(), count, sc->opt, nullptr, one.data())
              : single_check_group(lead, s, ms.data(), count, sc->opt, nullptr, one.data()));
  for (int z = 0; z < count; ++z) {
    if (!one[z]) continue;
    Member& m = mb[z];
    m.state = 2;
    std::fill(labels[m.index], labels[m.index] + ns[m.index], (int64_t)0);
    if (diags) memset(diags + m.index, 0, sizeof(sc_diag));
    if (sc->single) sc->single[m.index] = 1;
    if (lead->groutes) lead->groutes[m.index] = route;
  }
  return SC_OK;
}

// Eigensolver and k-means of a group whose stages before are enqueued (enqueue_front), in
// lockstep on the owner's stream; then the members that left the common path.
int finish_group(sc_handle lead, const int* ns, const sc_config* cfg, int64_t* const* labels,
                 sc_diag* diags, Member* mb, int count, const EigRequest& rq, int front_bank,
                 const SingleCheck* sc = nullptr) {
  const bool trace = sw::group_trace();
  SC_TRY(decide_single(lead, ns, labels, diags, mb, count, front_bank, false,
                       SC_BATCH_ROUTE_GROUP_LANCZOS, sc));
  // ---- eigen: lockstep over the symmetric members
  GroupEigMember em[kGroupMax];
  int emz[kGroupMax], ne = 0;
  SC_TRY(take_front(lead, ns, mb, count, rq, front_bank, em, emz, &ne));
  const double t1 = trace ? now_us() : 0.0;
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
                      GroupEigMember* em, int front_bank = -1, const SingleCheck* sc = nullptr) {
  const bool trace = sw::group_trace();
  SC_TRY(decide_single(lead, ns, labels, diags, mb, count, front_bank, true,
                       SC_BATCH_ROUTE_GROUP_JACOBI, sc));
  std::vector<int> emz(count);
  int ne = 0;  // (front_bank >= 0: the wave front, one event for the wave)
  SC_TRY(take_front(lead, ns, mb, count, rq, front_bank, em, emz.data(), &ne));
  const double t1 = trace ? now_us() : 0.0;
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

// The short members of a batch (`list`: indices sorted by n, descending) in waves of kShortWidth
// on the caller's handle and host thread.
int run_short_route(sc_handle h, const sc_array* xs, const int* ns, int d,
                    const sc_config* cfg, int64_t* const* labels, sc_diag* diags,
                    const std::vector<int>& list, const EigRequest& rq, const Bands* bands,
                    const SingleCheck* sc = nullptr) {
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
  const bool wave = !sw::short_front_memberwise() && !bands &&
                    d <= kShortWaveMaxD && short_wave_covers(cfg, &wave_ops);
  // (the grouped chain of a wave, the grouped ingest of callers' affinities: a stream of the wave's bank)
  if (wave || (bands && (bands->chain || bands->affinities || bands->dense)))
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
                             em.data(), wave ? j % banks : -1, sc);
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

// One lane of the grouped batch: the groups `mine` (indices into the size-sorted list, `width`
// members each) on the lead's streams and member arenas.
int run_group_lane(sc_handle h, const sc_array* xs, const int* ns, int d,
                   const sc_config* cfg, int64_t* const* labels, sc_diag* diags,
                   const std::vector<int>& grouped, const std::vector<int>& gstart, int width,
                   const std::vector<int>& mine, const EigRequest& rq, int group_limit,
                   const Bands* bands, const SingleCheck* sc = nullptr) {
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
                        front_bank[j % banks], sc));
  }
  return SC_OK;
}

// The members of a constrained batch that run as single calls on the caller's handle: each with
// its own band, entry list or dense matrix resident for the call (sc_predict with
// sc_set_constraint_band / sc_set_constraint_pairs / sc_set_constraint_array in front).
int predict_single_banded(sc_handle h, const std::vector<int>& list, const sc_array* xs,
                          const sc_config* cfg, int64_t* const* labels, sc_diag* diags,
                          const Bands& bands) {
  for (int i : list) {
    const int n = (int)xs[i].rows;
    if (bands.is_dense(i)) SC_TRY(sc_set_constraint_array(h, bands.dense + i));
    else if (bands.pairs(i))
      SC_TRY(sc_set_constraint_pairs(h, bands.cons[i].rows, bands.cons[i].cols, bands.cons[i].vals,
                                     bands.cons[i].count, n));
    else if (bands.band(i)) SC_TRY(sc_set_constraint_band(h, bands.band(i), n));
    else SC_TRY(sc_clear_constraint(h));
    h->sweep_slot.clear();
    if (bands.affinities) {  // (sc_predict_affinity_array behind the constraint)
      SC_TRY(sc_set_affinity_array(h, xs + i));
      SC_TRY(run_resident(h, cfg, labels[i], diags ? diags + i : nullptr, false));
      continue;
    }
    SC_TRY(ingest_embeddings(h, xs[i], xs[i].location == SC_MEM_HOST));
    SC_TRY(sc_run_resident(h, cfg, labels[i], diags ? diags + i : nullptr));
  }
  return sc_clear_constraint(h);
}

// The members of a min_clusters = 1 batch that run as single calls on the caller's handle: the
// affinity, the single call's own decision on it (sc_affinity_stats / sc_affinity_gmm_bic's code),
// and for a member of several clusters the eigensolver and k-means -- predict()'s sequence.
int predict_single_checked(sc_handle h, const std::vector<int>& list, const sc_array* xs,
                           const int* ns, const sc_config* cfg, int64_t* const* labels,
                           sc_diag* diags, const SingleCheck& sc) {
  for (int i : list) {
    h->sweep_slot.clear();
    SC_TRY(ingest_embeddings(h, xs[i], xs[i].location == SC_MEM_HOST));
    sc_diag local;
    sc_diag* dg = diags ? diags + i : &local;
    memset(dg, 0, sizeof(*dg));
    h->nev = 0;
    SC_TRY(sc_compute_affinity(h));
    int32_t one = 0;
    SC_TRY(single_check_resident(h, sc.opt, nullptr, &one));
    if (one) {
      std::fill(labels[i], labels[i] + ns[i], (int64_t)0);
      if (sc.single) sc.single[i] = 1;
      continue;
    }
    SC_TRY(eig_ncluster_impl(h, cfg, dg, nullptr));
    int k = dg->n_clusters_raw;
    if (cfg->min_clusters > 0 && k < cfg->min_clusters) k = cfg->min_clusters;  // :295-296
    SC_TRY(sc_cluster(h, cfg, k, labels[i], dg));
  }
  return SC_OK;
}

// Do the cp[] work matrices of a constrained batch fit?  Worst case: every position of both
// banks of the Lanczos route at the largest grouped member, every position of both wave banks of
// the short route at kDenseMax (what the arenas below reserve); what the arenas already hold counts.
// `stage_bytes`: the staging of the host dense sources of one front, worst case (the first arena
// of each bank holds it).
bool constraint_workspace_fits(sc_handle h, const Bands& bands, int largest, bool any_short,
                               size_t stage_bytes) {
  if (bands.ncp == 0 && !bands.dense) return true;
  auto need = [&](const std::vector<sc_handle_s*>& slots, int positions, int n) {
    const size_t nn = (size_t)n * matrix_ld(n) * sizeof(double);
    size_t bytes = 0;
    for (int z = 0; z < positions; ++z) {
      for (int i = 0; i < bands.ncp; ++i) {
        const size_t have = z < (int)slots.size() ? slots[z]->cp[i].bytes : 0;
        if (have < nn) bytes += nn;
      }
      // (a batch with a dense member: one more matrix per position, the arena's Cq)
      if (bands.dense && (z < (int)slots.size() ? slots[z]->Cq.bytes : 0) < nn) bytes += nn;
    }
    return bytes;
  };
  size_t bytes = 0;
  if (largest > 0) bytes += need(h->gslots, kGroupBanks * kGroupMax, largest);
  if (any_short) bytes += need(h->gshort, kGroupBanks * kShortWidth, kDenseMax);
  bytes += kGroupBanks * stage_bytes;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
  return (double)bytes <= 0.85 * (double)free_b;
}

// partition, groups, lanes, banks and short waves of a grouped batch; `band_set.cons` non-null:
// the constrained batch (one lane, member-by-member fronts, enqueue_front's band handling)
int predict_batch_core(sc_handle h, const sc_array* xs, const int* ns, int d, int count,
                       const sc_config* cfg, int64_t* const* labels, sc_diag* diags, int group,
                       const Bands& band_set, const SingleCheck* sc = nullptr) {
  const Bands* bands =
      band_set.cons || band_set.affinities || band_set.dense ? &band_set : nullptr;
  if (sc && sc->single) std::fill(sc->single, sc->single + count, 0);
  SC_TRY(validate_config(h, cfg));
  SC_HIP(h, hipSetDevice(h->device));
  group = std::max(1, std::min(group, kGroupMax));
  // the batch reuses the member arenas a sweep may have left eigenvectors in
  h->sweep_slot.clear();
  for (sc_handle lane : h->glanes) lane->sweep_slot.clear();
  const EigRequest rq = make_eig_request(cfg);
  // the chain's iteration kernel takes every device metric: cosine without being asked, the
  // others with the handle's permission (sc_set_batch_any_metric); a code that names no metric
  // goes to the single call, which says so
  const bool metric_ok =
      cfg->kmeans_metric == kKmeansCosine ||
      (h->batch_any_metric && cfg->kmeans_metric > kKmeansCosine &&
       cfg->kmeans_metric <= kKmeansCanberra);
  const bool cfg_ok = group > 1 && metric_ok &&
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
    // (the chain form of the single-cluster test covers n < kScChainMaxN, the route's own limit
    //  unless a switch has moved that)
    // (an entry list longer than n takes the dense stage: the single call's)
    if (bands && bands->pairs(i) && bands->cons[i].count > ns[i])
      single.push_back(i);
    else if (cfg_ok && xs[i].data && ns[i] > 0 && sym_group_eligible(ns[i], rq) &&
             (!sc || ns[i] < kScChainMaxN))
      grouped.push_back(i);
    else if (cfg_ok && xs[i].data && ns[i] > 0 && ns[i] <= kDenseMax) shorts.push_back(i);
    else single.push_back(i);
  }
  if (bands) {
    // the chain's work matrices are reserved with the arenas, before the first front: when they
    // do not fit, the members that carry a band run as single calls instead
    int largest = 0;
    bool any_short = false;
    for (int i : grouped) largest = std::max(largest, ns[i]);
    for (int i : shorts) any_short = any_short || bands->has(i);
    // a front's host dense sources are staged at their own width: at most `group` members of a
    // lockstep group, each no larger than the largest one, or a wave's kShortWidth of n <= kDenseMax
    size_t stage_one = 0, stage_short = 0;
    auto staged = [&](int i) {
      return bands->is_dense(i) && bands->dense[i].location == SC_MEM_HOST
                 ? affinity_group_stage_bytes(bands->dense + i, 1) : (size_t)0;
    };
    for (int i : grouped) stage_one = std::max(stage_one, staged(i));
    for (int i : shorts) stage_short = std::max(stage_short, staged(i));
    const size_t stage_bytes = std::max((size_t)group * stage_one, (size_t)kShortWidth * stage_short);
    if (!constraint_workspace_fits(h, *bands, largest, any_short, stage_bytes)) {
      auto hand_over = [&](std::vector<int>& list) {
        std::vector<int> keep;
        for (int i : list) (bands->has(i) ? single : keep).push_back(i);
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
    std::vector<int> gstart;
    int width = std::min(group, (int)grouped.size());
    const int min_groups = ((int)grouped.size() + width - 1) / width;
    const int lanes_wanted = std::max(
        1, std::min(kGroupLanes, covered ? min_groups / kGroupBanks : 1));
    if (min_groups < 2) {
      for (int at = 0; at < (int)grouped.size(); at += width) gstart.push_back(at);
    } else {
      double total = 0.0;
      for (int i : grouped) total += unit_cost(ns[i]);
      const int per_lane = std::max(kGroupBanks, (min_groups + lanes_wanted - 1) / lanes_wanted);
      const int target_groups = lanes_wanted * per_lane;
      const double share = total / target_groups;
      double run = 0.0;
      int start = 0;
      for (int at = 0; at < (int)grouped.size(); ++at) {
        const double c = unit_cost(ns[grouped[at]]);
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
        for (int at = gstart[g]; at < gstart[g + 1]; ++at) gcost[g] += unit_cost(ns[grouped[at]]);
      std::vector<int> order(ngroups);
      for (int g = 0; g < ngroups; ++g) order[g] = g;
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return gcost[a] > gcost[b]; });
      deal_least_loaded(order, [&](int g) { return gcost[g]; }, lanes, lane_groups);
    }
    sc_handle leads[kGroupLanes] = {h};
    SC_TRY(ensure_lanes(h, lanes, "grouped batch", leads));  // (they report into h->groutes)
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
    auto run_lane = [&](int l) {
      return run_group_lane(leads[l], xs, ns, d, cfg, labels, diags, grouped, gstart, width,
                            lane_groups[l], rq, group, bands, sc);
    };
    for (int l = 1; l < lanes; ++l) {
      auto body = [&, l]() {
        if (hipSetDevice(h->device) != hipSuccess) {
          rcs[l] = fail(leads[l], SC_ERR_HIP, "hipSetDevice failed on a lane");
          return;
        }
        rcs[l] = run_lane(l);
      };
      try {
        side.emplace_back(body);
      } catch (...) {  // (no thread to be had: the lane runs on this one, after lane 0)
        inline_lane[l] = true;
      }
    }
    rcs[0] = run_lane(0);
    for (int l = 1; l < lanes; ++l)
      if (inline_lane[l]) rcs[l] = run_lane(l);
    for (auto& t : side) t.join();
    // (the lanes keep up to 3 x 2 x 16 member arenas warm otherwise: 21 GB after config 5)
    release_large_arenas(leads, lanes);
    if (rcs[0] != SC_OK) return rcs[0];
    for (int l = 1; l < lanes; ++l)
      if (rcs[l] != SC_OK) return fail(h, rcs[l], leads[l]->err.c_str());
  }
  // the short route (n <= kDenseMax), once the lanes of the Lanczos route are done: waves of
  // kShortWidth members, largest first (a wave's Jacobi launch lasts as long as its largest member)
  if (!shorts.empty()) {
    std::stable_sort(shorts.begin(), shorts.end(), [&](int a, int b) { return ns[a] > ns[b]; });
    SC_TRY(run_short_route(h, xs, ns, d, cfg, labels, diags, shorts, rq, bands, sc));
  }
  // (members outside the grouped path's range -- n >= 4096 above all: their uploads ride under
  //  the previous member's pipeline, api.hip predict_sequence)
  if (!single.empty() && sc)
    SC_TRY(predict_single_checked(h, single, xs, ns, cfg, labels, diags, *sc));
  else if (!single.empty() && bands)
    SC_TRY(predict_single_banded(h, single, xs, cfg, labels, diags, *bands));
  else if (!single.empty())
    SC_TRY(predict_sequence(h, single.data(), (int)single.size(), xs, ns, d, cfg, labels, diags));
  return SC_OK;
}
}  // namespace

// ---- what the sweep, the AutoTune batch and the stage hook use as well (batch_internal.h)
constexpr int kRndStride = 256;  // doubles per k in the RandomState(0) table (k <= 32)

int group_slot(sc_handle lead, int z, sc_handle* out, std::vector<sc_handle_s*>* arenas) {
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

// ---- launch descriptors of a member arena (batch_internal.h says what each one names)
FrontItem front_item(sc_handle h, int parts) {
  FrontItem f;
  memset(&f, 0, sizeof(f));
  f.n = h->n;
  f.ldn = h->ldn;
  f.flags = ptr<int>(h->flags);
  if (parts & kFrontRows) {
    f.X = ptr<double>(h->X);
    f.Xn = ptr<double>(h->Xn);
    f.ldx = h->ldx;
    f.d = h->d;
    f.symflag = ptr<int>(h->symflag);
  }
  if (parts & kFrontSource) {
    f.A0 = ptr<double>(h->A0);
    f.cropval = ptr<double>(h->cropval);
    f.B1 = ptr<double>(h->B1);
    f.rmpart = ptr<double>(h->rmpart);
  }
  if (parts & kFrontRefined) {
    f.B2 = ptr<double>(h->B2);
    f.cut = ptr<double>(h->cut);
    f.rowmax = ptr<double>(h->rowmax);
    f.rowsum = ptr<double>(h->rowsum);
    f.cvec = ptr<double>(h->cvec);
    f.pvec = ptr<double>(h->pvec);
    f.tvec = ptr<double>(h->tvec);
  }
  return f;
}
GemmGroupItem affinity_item(sc_handle h) {
  GemmGroupItem g;
  g.A = ptr<double>(h->Xn);
  g.lda = h->ldx;
  g.C = ptr<double>(h->A0);
  g.ldc = h->ldn;
  g.n = h->n;
  g.K = h->d;
  g.tilemap = h->tilemap_cur;
  g.partial_max = ptr<double>(h->statp);
  return g;
}
GemmGroupItem diffuse_item(sc_handle h, bool reduced_stats) {
  GemmGroupItem g;
  g.A = ptr<double>(h->B2);
  g.lda = h->ldn;
  g.C = ptr<double>(h->B1);
  g.ldc = h->ldn;
  g.n = h->n;
  g.K = h->n;
  g.tilemap = h->tilemap_cur;
  g.partial_max = ptr<double>(h->statp);
  g.partial_sum = ptr<double>(h->statp) + (size_t)h->n * gemm_tile_dim(h->n);
  if (reduced_stats) {
    g.rowmax = ptr<double>(h->rowmax);
    g.rowsum = ptr<double>(h->rowsum);
  }
  return g;
}
ShortWaveItem short_wave_item(sc_handle h) {
  ShortWaveItem it;
  it.n = h->n;
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
  return it;
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
    const int n = ns[m.index];
    SC_TRY(member_problem(lead, h, xs[m.index], n, d, s));
    h->have_cropval = true;  // (out of the affinity epilogue, below)
    if (diags) memset(diags + m.index, 0, sizeof(sc_diag));
    FrontItem& f = fi[z];
    f = front_item(h, kFrontRows | kFrontSource | kFrontRefined);
    f.blur_cols = blur_stream_columns(n, cfg->blur_radius);  // (the grouped front streams)
    aff[z] = affinity_item(h);
    aff[z].rowmax = ptr<double>(h->cropval);  // the launch folds the partials: CropDiagonal's value
    m.front.crop_source = 1;  // (the affinity epilogue writes the value the blur reads)
    dif[z] = diffuse_item(h, true);
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
      const int rc = ensure_free(h, n);
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
    const int n = ns[m.index];
    if (n > kDenseMax) return fail(lead, SC_ERR_INVALID, "short wave: a member above 128 rows");
    SC_TRY(member_problem(lead, h, xs[m.index], n, d, s));
    h->have_cropval = ops.crop != 0;  // (the front kernel writes the vector only then)
    h->have_constraint = h->constraint_banded = h->constraint_pairs = false;  // (a constrained
    // wave's arena: its band or entry list)
    h->qn = 0;
    if (diags) memset(diags + m.index, 0, sizeof(sc_diag));
    fi[z] = front_item(h, kFrontRows);  // (the rest is the wave kernel's, which reads the table)
    aff[z] = affinity_item(h);  // (rowmax stays null: the wave kernel folds the one tile's partials)
    dif[z] = diffuse_item(h, false);  // (likewise: launch_short_wave_scaling reads statp)
    htab[z] = short_wave_item(h);
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
// whose solve or cluster count left the common path gets state 1 (single_path_members).
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
    it.metric = cfg->kmeans_metric;
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

int ensure_lanes(sc_handle h, int lanes, const char* what, sc_handle* leads) {
  leads[0] = h;
  for (int l = 1; l < lanes; ++l) {
    while ((int)h->glanes.size() < l) {
      sc_handle lane = nullptr;
      const int rc = sc_create(h->device, &lane);
      if (rc != SC_OK) return fail(h, rc, std::string("could not create a lane of the ") + what);
      lane->profile_level = 1;
      h->glanes.push_back(lane);
    }
    leads[l] = h->glanes[l - 1];
    leads[l]->blur_ext = h->blur_ext;
    leads[l]->err.clear();
    leads[l]->groutes = h->groutes;
  }
  return SC_OK;
}

bool release_large_arenas(sc_handle* leads, int lanes, bool always) {
  size_t free_b = 0, total_b = 0, held = 0;
  if (!always) {
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
    for (int l = 0; l < lanes; ++l)
      for (sc_handle sub : leads[l]->gslots) {
        held += sub->A0.bytes + sub->B1.bytes + sub->B2.bytes;
        for (const DevBuf& w : sub->cp) held += w.bytes;  // (a constrained batch's work matrices,
        held += sub->Cq.bytes + sub->Xstage.bytes;        //  dense constraints and their staging)
      }
    if (held <= total_b / 4) return false;
  }
  for (int l = 0; l < lanes; ++l) {
    for (sc_handle sub : leads[l]->gslots) sc_destroy(sub);
    leads[l]->gslots.clear();
    leads[l]->sweep_slot.clear();
  }
  return true;
}

extern "C" int sc_constraint_desc_layout(int* bytes, int* field_offsets) {
  if (bytes) *bytes = (int)sizeof(sc_constraint_desc);
  if (field_offsets) {
    field_offsets[0] = (int)offsetof(sc_constraint_desc, kind);
    field_offsets[1] = (int)offsetof(sc_constraint_desc, count);
    field_offsets[2] = (int)offsetof(sc_constraint_desc, band);
    field_offsets[3] = (int)offsetof(sc_constraint_desc, rows);
    field_offsets[4] = (int)offsetof(sc_constraint_desc, cols);
    field_offsets[5] = (int)offsetof(sc_constraint_desc, vals);
  }
  return SC_OK;
}

extern "C" int sc_predict_batch_constraints(sc_handle h, const sc_array* xs,
                                            const sc_constraint_desc* cons, int count,
                                            const sc_config* cfg, int64_t* const* labels,
                                            sc_diag* diags, int group) {
  if (!h) return SC_ERR_INVALID;
  if (!xs || !labels || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  if (group < 2)
    return fail(h, SC_ERR_INVALID, "a constrained batch is the grouped form: group >= 2");
  SC_TRY(validate_config(h, cfg));
  SC_HIP(h, hipSetDevice(h->device));
  bool device_source = false;
  std::vector<int> ns;
  int d = 0;
  SC_TRY(validate_batch_arrays(h, xs, count, &ns, &d, &device_source));
  SC_TRY(sc_clear_constraint(h));  // the handle's own resident constraint takes no part
  if (count == 0) {
    h->last_routes.clear();
    return SC_OK;
  }
  if (device_source) SC_HIP(h, hipStreamSynchronize(h->stream));  // (as sc_predict_batch_arrays)
  return predict_batch_constrained_impl(h, xs, cons, ns.data(), d, count, cfg, labels, diags,
                                        group);
}

// (sc_predict_batch_constraints with every kind 0 or 2)
extern "C" int sc_predict_batch_constrained(sc_handle h, const sc_array* xs,
                                            const double* const* bands, int count,
                                            const sc_config* cfg, int64_t* const* labels,
                                            sc_diag* diags, int group) {
  if (!h) return SC_ERR_INVALID;
  if (!xs || !labels || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  if (group < 2)
    return fail(h, SC_ERR_INVALID, "sc_predict_batch_constrained is the grouped form: group >= 2");
  std::vector<sc_constraint_desc> cons;
  if (bands && count > 0) {
    cons.assign((size_t)count, sc_constraint_desc());
    for (int i = 0; i < count; ++i) {
      cons[i].kind = bands[i] ? 2 : 0;
      cons[i].band = bands[i];
    }
  }
  return sc_predict_batch_constraints(h, xs, cons.empty() ? nullptr : cons.data(), count, cfg,
                                      labels, diags, group);
}

int predict_batch_constrained_impl(sc_handle h, const sc_array* xs, const sc_constraint_desc* cons,
                                   const int* ns, int d, int count, const sc_config* cfg,
                                   int64_t* const* labels, sc_diag* diags, int group,
                                   bool affinities, const sc_array* dense) {
  // every entry list is checked, and packed for its upload, before anything is launched
  std::vector<std::vector<double>> packed((size_t)count);
  std::vector<char> pairs_symmetric((size_t)count, 1);
  int kmax = 0;
  const bool read = cons && cfg->constraint_name != SC_CONSTRAINT_NONE;
  for (int i = 0; read && i < count; ++i) {
    const sc_constraint_desc& c = cons[i];
    if (c.kind != 0 && c.kind != 2 && c.kind != 3)
      return fail(h, SC_ERR_INVALID, "constraint kind must be 0 (none), 2 (band) or 3 (pairs)");
    if (c.kind == 2 && !c.band)
      return fail(h, SC_ERR_INVALID, "a band constraint without its values");
    if (c.kind != 3) continue;
    bool symmetric = true;
    SC_TRY(validate_constraint_pairs(h, c.rows, c.cols, c.vals, c.count, ns[i], &symmetric));
    pairs_symmetric[i] = symmetric ? 1 : 0;
    if (c.count > ns[i]) continue;  // (the dense stage: a single call, sc_set_constraint_pairs)
    packed[i] = pack_constraint_pairs(c.rows, c.cols, c.vals, c.count);
    kmax = std::max(kmax, std::max(c.count, 1));  // (an empty list still reserves its buffers)
  }
  // no constraint stays resident in a member arena, and none of them is still on its way up from
  // the caller's memory, however the batch ends
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
  Bands bands = make_bands(cons, packed.data(), pairs_symmetric.data(), kmax, cfg, dense);
  bands.affinities = affinities;
  cleanup.rc = predict_batch_core(h, xs, ns, d, count, cfg, labels, diags, group, bands);
  return cleanup.rc;
}

extern "C" int sc_predict_batch_affinities(sc_handle h, const sc_array* as,
                                           const sc_constraint_desc* cons, int count,
                                           const sc_config* cfg, int64_t* const* labels,
                                           sc_diag* diags, int group) {
  if (!h) return SC_ERR_INVALID;
  if (!as || !labels || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  if (group < 2)
    return fail(h, SC_ERR_INVALID, "sc_predict_batch_affinities is the grouped form: group >= 2");
  SC_TRY(validate_config(h, cfg));
  SC_HIP(h, hipSetDevice(h->device));
  bool device_source = false;
  std::vector<int> ns(count, 0);
  for (int i = 0; i < count; ++i) {  // every descriptor before the first launch
    SC_TRY(validate_affinity_array(h, as + i));
    if (!labels[i]) return fail(h, SC_ERR_INVALID, "NULL labels");
    ns[i] = (int)as[i].rows;
    device_source |= as[i].location == SC_MEM_DEVICE;
  }
  if (count == 0) {
    h->last_routes.clear();
    return SC_OK;
  }
  // (as sc_predict_batch_arrays: what the producers ordered before this stream is done before
  //  the streams of the batch read a device source)
  if (device_source) SC_HIP(h, hipStreamSynchronize(h->stream));
  SC_TRY(sc_clear_constraint(h));  // the handle's own resident constraint takes no part
  return predict_batch_constrained_impl(h, as, cons, ns.data(), 0, count, cfg, labels, diags, group,
                                        true);
}

extern "C" int sc_predict_batch_constraint_arrays(sc_handle h, const sc_array* xs,
                                                  const sc_constraint_desc* cons,
                                                  const sc_array* dense, int count,
                                                  const sc_config* cfg, int64_t* const* labels,
                                                  sc_diag* diags, int group, int affinities) {
  if (!h) return SC_ERR_INVALID;
  if (!dense)  // exactly the existing calls
    return affinities ? sc_predict_batch_affinities(h, xs, cons, count, cfg, labels, diags, group)
                      : sc_predict_batch_constraints(h, xs, cons, count, cfg, labels, diags, group);
  if (!xs || !labels || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  if (group < 2)
    return fail(h, SC_ERR_INVALID,
                "sc_predict_batch_constraint_arrays is the grouped form: group >= 2");
  SC_TRY(validate_config(h, cfg));
  SC_HIP(h, hipSetDevice(h->device));
  bool device_source = false;
  std::vector<int> ns(count, 0);
  int d = 0;
  if (affinities) {
    for (int i = 0; i < count; ++i) {  // every descriptor before the first launch
      SC_TRY(validate_affinity_array(h, xs + i));
      ns[i] = (int)xs[i].rows;
      device_source |= xs[i].location == SC_MEM_DEVICE;
    }
  } else {
    SC_TRY(validate_batch_arrays(h, xs, count, &ns, &d, &device_source));
  }
  bool any_dense = false;
  for (int i = 0; i < count; ++i) {
    if (!labels[i]) return fail(h, SC_ERR_INVALID, "NULL labels");
    if (!dense[i].data) continue;
    if (cons && cons[i].kind != 0)
      return fail(h, SC_ERR_INVALID, "an utterance with a dense constraint has constraint kind 0");
    SC_TRY(validate_affinity_array(h, dense + i, "constraint matrix"));
    if (dense[i].rows != ns[i])
      return fail(h, SC_ERR_INVALID, "affinity and constraint matrix must have the same shape");
    any_dense = true;
    device_source |= dense[i].location == SC_MEM_DEVICE;
  }
  SC_TRY(sc_clear_constraint(h));  // the handle's own resident constraint takes no part
  if (count == 0) {
    h->last_routes.clear();
    return SC_OK;
  }
  if (device_source) SC_HIP(h, hipStreamSynchronize(h->stream));  // (as sc_predict_batch_arrays)
  return predict_batch_constrained_impl(h, xs, cons, ns.data(), d, count, cfg, labels, diags,
                                        group, affinities != 0, any_dense ? dense : nullptr);
}

extern "C" int sc_predict_batch_single(sc_handle h, const sc_array* xs, int count,
                                       const sc_config* cfg, const sc_single_check* check,
                                       int64_t* const* labels, sc_diag* diags, int group,
                                       int32_t* single) {
  if (!h) return SC_ERR_INVALID;
  if (!xs || !labels || count < 0) return fail(h, SC_ERR_INVALID, "NULL argument");
  if (group < 2)
    return fail(h, SC_ERR_INVALID, "sc_predict_batch_single is the grouped form: group >= 2");
  SC_TRY(validate_config(h, cfg));
  if (check) SC_TRY(validate_single_check(h, check));
  SC_HIP(h, hipSetDevice(h->device));
  bool device_source = false;
  std::vector<int> ns;
  int d = 0;
  SC_TRY(validate_batch_arrays(h, xs, count, &ns, &d, &device_source));
  // (sc_affinity_gmm_bic's check, for every utterance before anything is launched)
  for (int i = 0; check && i < count; ++i) SC_TRY(check_single_offset(h, check, ns[i], i));
  if (count == 0) {
    h->last_routes.clear();
    return SC_OK;
  }
  if (device_source) SC_HIP(h, hipStreamSynchronize(h->stream));  // (as sc_predict_batch_arrays)
  return predict_batch_single_impl(h, xs, ns.data(), d, count, cfg, check, labels, diags, group,
                                   single);
}

int predict_batch_single_impl(sc_handle h, const sc_array* xs, const int* ns, int d, int count,
                              const sc_config* cfg, const sc_single_check* check,
                              int64_t* const* labels, sc_diag* diags, int group,
                              int32_t* single) {
  SingleCheck sc;
  sc.opt = check;
  sc.single = single;
  if (!check && single) std::fill(single, single + count, 0);
  return predict_batch_core(h, xs, ns, d, count, cfg, labels, diags, group, Bands(),
                            check ? &sc : nullptr);
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
