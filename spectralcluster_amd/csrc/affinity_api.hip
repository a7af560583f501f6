// An affinity the caller already holds comes in where it is: a described (n, n) array (sc_array:
// device or host memory, fp64 / fp32 / fp16 / bf16, any element strides) becomes the handle's
// resident affinity A0 -- widened exactly by k_ingest_affinity (ingest.hip), which decides the
// matrix's symmetry in the same pass.  Everything behind the affinity (constraints, refinement,
// eigensolver, sweep, k-means) already works from a resident matrix that was not made from
// embeddings (affinity_from_embeddings = false).
#include "handle.h"

namespace {

// sc_set_affinity's state for a described source.  `nan_fill`: the destination is filled with
// NaNs first (the test entry shows what the ingest wrote).
int set_affinity_array(sc_handle h, const sc_array* a, bool nan_fill) {
  SC_TRY(validate_affinity_array(h, a));
  SC_HIP(h, hipSetDevice(h->device));
  const int n = (int)a->rows;
  SC_TRY(ensure_matrices(h, n, 0));
  SC_TRY(grow(h, h->symflag, 16));
  h->n = n;
  h->ldn = matrix_ld(n);
  h->have_x = false;
  h->have_affinity = false;
  h->n_vec = 0;
  h->sweep_slot.clear();
  if (nan_fill)
    SC_HIP(h, hipMemsetAsync(h->A0.p, 0xff, (size_t)n * h->ldn * sizeof(double), h->stream));
  bool sync = false;
  SC_TRY(ingest_affinity_into(h, *a, ptr<double>(h->A0), h->ldn, ptr<int>(h->symflag), h->stream,
                              &sync));
  // the flag is read here, whatever the sequence does with it later: the wait also is the
  // promise that the source may be reused (sc_set_affinity makes the same one)
  int symmetric = 0;
  SC_HIP(h, hipMemcpyAsync(&symmetric, h->symflag.p, sizeof(int), hipMemcpyDeviceToHost,
                           h->stream));
  SC_HIP(h, hipStreamSynchronize(h->stream));
  h->affinity_symmetric = symmetric != 0;
  h->have_affinity = true;
  h->have_cropval = false;
  h->constraint_applied = false;
  h->affinity_from_embeddings = false;
  return SC_OK;
}

}  // namespace

extern "C" int sc_set_affinity_array(sc_handle h, const sc_array* a) {
  if (!h) return SC_ERR_INVALID;
  return set_affinity_array(h, a, false);
}

extern "C" int sc_predict_affinity_array(sc_handle h, const sc_array* a, const sc_config* cfg,
                                         int64_t* labels, sc_diag* diag) {
  if (!h) return SC_ERR_INVALID;
  SC_TRY(validate_config(h, cfg));
  if (!labels) return fail(h, SC_ERR_INVALID, "labels is NULL");
  SC_TRY(set_affinity_array(h, a, false));
  return run_resident(h, cfg, labels, diag, false);
}

extern "C" int sc_stage_affinity_ingest(sc_handle h, const sc_array* a, double* out,
                                        int* symmetric) {
  if (!h) return SC_ERR_INVALID;
  if (!out || !symmetric) return fail(h, SC_ERR_INVALID, "out / symmetric is NULL");
  SC_TRY(set_affinity_array(h, a, true));
  *symmetric = h->affinity_symmetric ? 1 : 0;
  return d2h_matrix(h, ptr<double>(h->A0), h->ldn, h->n, h->ldn, out);
}

extern "C" int sc_stage_affinity_ingest_group(sc_handle h, const sc_array* as, int count,
                                              double* const* outs, int* symmetric) {
  if (!h) return SC_ERR_INVALID;
  if (!as || !outs || !symmetric || count <= 0 || count > 64)
    return fail(h, SC_ERR_INVALID, "1 .. 64 affinities, outs and symmetric");
  for (int z = 0; z < count; ++z) {  // every descriptor before the first launch
    SC_TRY(validate_affinity_array(h, as + z));
    if (!outs[z]) return fail(h, SC_ERR_INVALID, "NULL out");
  }
  SC_HIP(h, hipSetDevice(h->device));
  // one allocation of the call's own: [flags | table | stage | member 0 | member 1 | ...]
  auto align256 = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t flags_at = 0, table_at = align256(count * sizeof(int));
  const size_t stage_at = table_at + align256(count * affinity_group_table_bytes());
  size_t total = stage_at + align256(affinity_group_stage_bytes(as, count));
  std::vector<size_t> member_at(count);
  for (int z = 0; z < count; ++z) {
    member_at[z] = total;
    total += align256((size_t)as[z].rows * matrix_ld((int)as[z].rows) * sizeof(double));
  }
  unsigned char* base = nullptr;
  SC_HIP(h, hipMalloc(reinterpret_cast<void**>(&base), total));
  std::vector<double*> dsts(count);
  for (int z = 0; z < count; ++z) dsts[z] = reinterpret_cast<double*>(base + member_at[z]);
  auto run = [&]() -> int {
    SC_HIP(h, hipMemsetAsync(base + member_at[0], 0xff, total - member_at[0], h->stream));
    SC_TRY(ingest_affinity_group(h, as, count, dsts.data(),
                                 reinterpret_cast<int*>(base + flags_at), base + stage_at,
                                 base + table_at, h->stream));
    SC_HIP(h, hipMemcpyAsync(symmetric, base + flags_at, count * sizeof(int),
                             hipMemcpyDeviceToHost, h->stream));
    for (int z = 0; z < count; ++z) {
      const int n = (int)as[z].rows, ld = matrix_ld(n);
      SC_TRY(d2h_matrix(h, dsts[z], ld, n, ld, outs[z]));
    }
    return SC_OK;
  };
  const int rc = run();
  hipStreamSynchronize(h->stream);
  hipFree(base);
  return rc;
}
