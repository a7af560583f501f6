/*
 * spectralcluster_amd.h -- C ABI of the MI355X (gfx950) implementation of the
 * dense hot path of SpectralClusterer.predict() (wq2012/SpectralCluster
 * v0.2.22).  Plain pointers and sizes only; no torch / numpy types.
 *
 * Every entry point names the reference interface it replaces (paths are
 * relative to the reference checkout, `spectralcluster/...`).  The reference
 * is pure Python, so "the binding a maintainer would add" is a ctypes stub;
 * see INTEGRATION.md.
 *
 * Conventions
 *   - all matrices are float64, C-contiguous row-major, caller-owned;
 *   - every function returns an sc_status (0 = ok, < 0 = error); the text
 *     of the last error of a handle is available from sc_last_error();
 *   - one handle <-> one device <-> one HIP stream.  A handle is NOT
 *     thread-safe; distinct handles are independent;
 *   - no host pointer is retained after a call returns.
 */
#ifndef SPECTRALCLUSTER_AMD_H_
#define SPECTRALCLUSTER_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_ABI_VERSION 11
#define SC_MAX_OPS 16
#define SC_MAX_BLUR_RADIUS 32
#define SC_MAX_EIG 128 /* max eigenvalues reported in sc_diag */
#define SC_MAX_STAGES 16

typedef struct sc_handle_s* sc_handle;

typedef enum sc_status {
  SC_OK = 0,
  SC_ERR_INVALID = -1,       /* bad argument (maps to ValueError/TypeError) */
  SC_ERR_OOM = -2,           /* device allocation failed */
  SC_ERR_HIP = -3,           /* HIP runtime error */
  SC_ERR_NOT_CONVERGED = -4, /* eigensolver did not reach tolerance */
  SC_ERR_UNSUPPORTED = -5,   /* configuration outside the device path */
  SC_ERR_NON_FINITE = -6     /* NaN / inf reached the eigen stage (numpy: LinAlgError) */
} sc_status;

/* refinement.py:11-18 RefinementName */
typedef enum sc_op {
  SC_OP_CROP_DIAGONAL = 1,
  SC_OP_GAUSSIAN_BLUR = 2,
  SC_OP_ROW_WISE_THRESHOLD = 3,
  SC_OP_SYMMETRIZE = 4,
  SC_OP_DIFFUSE = 5,
  SC_OP_ROW_WISE_NORMALIZE = 6
} sc_op;

/* refinement.py:21-27 ThresholdType, :30-36 SymmetrizeType */
enum { SC_THRESHOLD_ROW_MAX = 1, SC_THRESHOLD_PERCENTILE = 2 };
enum { SC_SYMMETRIZE_MAX = 1, SC_SYMMETRIZE_AVERAGE = 2 };
/* laplacian.py:9-21 LaplacianType (0 = laplacian_type None) */
enum {
  SC_LAPLACIAN_NONE = 0,
  SC_LAPLACIAN_AFFINITY = 1,
  SC_LAPLACIAN_UNNORMALIZED = 2,
  SC_LAPLACIAN_RANDOM_WALK = 3,
  SC_LAPLACIAN_GRAPH_CUT = 4
};
/* constraint.py:10-16 ConstraintName (0 = constraint_options None), :19-22 IntegrationType */
enum {
  SC_CONSTRAINT_NONE = 0,
  SC_CONSTRAINT_AFFINITY_INTEGRATION = 1,
  SC_CONSTRAINT_PROPAGATION = 2
};
enum { SC_INTEGRATION_MAX = 1, SC_INTEGRATION_AVERAGE = 2 };
/* linkage of the size-reduction / fallback agglomerative clustering */
enum { SC_LINKAGE_COMPLETE = 1, SC_LINKAGE_AVERAGE = 2 };
/* custom_dist of run_kmeans (custom_distance_kmeans.py:13-52): the scipy cdist metric
 * names that run on the device.  (A falsy custom_dist makes the reference call .predict()
 * on an unfitted sklearn KMeans, :33-36/:51 -- it always raises; the host side mirrors that.) */
enum {
  SC_KMEANS_COSINE = 0,
  SC_KMEANS_EUCLIDEAN = 1,
  SC_KMEANS_SQEUCLIDEAN = 2,
  SC_KMEANS_CITYBLOCK = 3,
  SC_KMEANS_CHEBYSHEV = 4,
  SC_KMEANS_CORRELATION = 5, /* cosine distance of the row-centred operands */
  SC_KMEANS_BRAYCURTIS = 6,
  SC_KMEANS_CANBERRA = 7
};
/* utils.py:10-17 EigenGapType */
enum { SC_EIGENGAP_RATIO = 1, SC_EIGENGAP_NORMALIZED_DIFF = 2 };

/* Which eigen path ran (sc_diag.eig_path) */
enum {
  SC_EIG_PATH_DENSE_JACOBI = 1,   /* symmetric, n <= 128 */
  SC_EIG_PATH_BLOCK_LANCZOS = 2,  /* symmetric, larger n */
  SC_EIG_PATH_DENSE_GENERAL = 3,  /* non-symmetric, n <= 64: Hessenberg + complex QR */
  SC_EIG_PATH_BLOCK_ARNOLDI = 4,  /* non-symmetric, larger n */
  /* symmetric, n > 128, every eigenvalue consumed (max_clusters=None with a Laplacian,
   * or the ascending NormalizedDiff gap's np.max): Householder tridiagonalisation +
   * Sturm bisection for the values, block Lanczos for the few vectors k-means takes */
  SC_EIG_PATH_DENSE_TRIDIAG = 5,
  /* block Lanczos gave up (sc_diag.eig_fallback says why): values as above and the vectors by
   * inverse iteration on the tridiagonal form + the Householder back-transform.  Always
   * returns, like np.linalg.eig (utils.py:59) */
  SC_EIG_PATH_DENSE_FULL = 6,
  /* non-symmetric, n > 64, when more eigenvalues are read than a block Arnoldi basis holds
   * (max_clusters=None with a Laplacian, max_clusters > 63, min_clusters > 64) or block Arnoldi
   * gives up: Householder reduction to Hessenberg form on the device, every eigenvalue by the
   * double-shift QR iteration and the eigenvectors k-means reads by inverse iteration on the
   * host.  Always returns, like np.linalg.eig (utils.py:59) */
  SC_EIG_PATH_DENSE_HESSENBERG = 7
};

/* Stage slots of sc_diag.stage_ms */
enum {
  SC_STAGE_AFFINITY = 0,
  SC_STAGE_REFINE = 1,    /* all refinement ops except Diffuse */
  SC_STAGE_DIFFUSE = 2,
  SC_STAGE_SCALING = 3,   /* row stats + Laplacian/normalise scaling vectors */
  SC_STAGE_EIG = 4,
  SC_STAGE_KMEANS = 5,
  SC_STAGE_TOTAL = 6,
  /* per-kernel slots, filled only at sc_set_profiling(h, 2) */
  SC_STAGE_BLUR = 7,           /* CropDiagonal + GaussianBlur kernel */
  SC_STAGE_THRESHOLD_SYM = 8,  /* RowWiseThreshold + Symmetrize kernel */
  SC_STAGE_MATVEC = 9,         /* sum over the block matvec launches of the eigen stage */
  SC_STAGE_AFFINITY_GEMM = 10, /* the affinity GEMM launch alone */
  /* matrix-free Diffuse (sc_diag.diffuse_path == SC_DIFFUSE_PATH_FREE); their sum is
   * SC_STAGE_DIFFUSE of such a call */
  SC_STAGE_FREE_QUANTIZE = 11, /* max|a| + 8-bit digits of A, rowsum(A) */
  SC_STAGE_FREE_PRODUCT = 12,  /* exact integer MFMA product of the digits */
  SC_STAGE_FREE_SCAN = 13,     /* row maxima + candidates within the proven slack */
  SC_STAGE_FREE_STATS = 14     /* exact fp64 rowmax(S) of the candidates, rowsum(S) */
};

/* How the last Diffuse (refinement.py:229-234) of the sequence ran (sc_diag.diffuse_path) */
enum {
  SC_DIFFUSE_PATH_NONE = 0,
  SC_DIFFUSE_PATH_EXPLICIT = 1,           /* S = A A^T by the fp64 MFMA GEMM */
  /* S never formed: rowmax(S) by the digit product + exact recheck, S V = A (A V) */
  SC_DIFFUSE_PATH_FREE = 2,
  /* started matrix-free, S formed after all (a dense eigen route read entries, or more rows
   * than the exact-row route takes had to be evaluated in full) */
  SC_DIFFUSE_PATH_FREE_THEN_EXPLICIT = 3
};

/*
 * POD mirror of SpectralClusterer.__init__ (spectral_clusterer.py:29-46) and
 * RefinementOptions (refinement.py:76-100), restricted to the hot path.
 * 0 means "None" for min_clusters / max_clusters.
 */
typedef struct sc_config {
  int32_t n_ops;                 /* len(refinement_sequence), 0 = no refinement */
  int32_t ops[SC_MAX_OPS];       /* sc_op values, applied in order */
  /* GaussianBlur: the 2*radius+1 symmetric weights as scipy computes them
   * (sigma -> radius int(4 sigma + .5)); radius 0 = plain copy (sigma == 0).
   * sc_gaussian_weights() fills these from sigma. */
  int32_t blur_radius;
  double blur_weights[2 * SC_MAX_BLUR_RADIUS + 1];
  double p_percentile;           /* refinement.py:79 */
  double soft_multiplier;        /* refinement.py:83 */
  int32_t threshold_type;        /* SC_THRESHOLD_* */
  int32_t binarize;              /* thresholding_with_binarization */
  int32_t preserve_diagonal;     /* thresholding_preserve_diagonal */
  int32_t symmetrize_type;       /* SC_SYMMETRIZE_* */
  int32_t laplacian_type;        /* SC_LAPLACIAN_* */
  int32_t min_clusters;          /* 0 = None */
  int32_t max_clusters;          /* 0 = None */
  double stop_eigenvalue;        /* spectral_clusterer.py:36 */
  int32_t eigengap_type;         /* SC_EIGENGAP_* */
  int32_t row_wise_renorm;       /* spectral_clusterer.py:37 */
  int32_t max_iter;              /* custom k-means iterations (:39) */
  /* Eigensolver knobs (no reference equivalent). 0 selects the default. */
  double eig_value_tol;          /* residual bound / |eigenvalue| on consumed values (1e-6) */
  double eig_vector_tol;         /* residual tol, relative to ||M||, on the
                                    eigenvectors handed to k-means (1e-10) */
  int32_t eig_max_cycles;        /* restart cycles block Lanczos may spend before the dense
                                    eigensolver takes over (0: default 40; < 0: none) */
  /* ConstraintOptions (constraint.py:26-48); used only while a constraint matrix
   * is resident (sc_set_constraint), like constraint_matrix=None in the reference */
  int32_t constraint_name;       /* SC_CONSTRAINT_* */
  int32_t constraint_before_refinement; /* apply_before_refinement */
  int32_t integration_type;      /* SC_INTEGRATION_* */
  double constraint_alpha;       /* constraint_propagation_alpha (0.6) */
  int32_t kmeans_metric;         /* SC_KMEANS_* (custom_dist, spectral_clusterer.py:38) */
  /* Route of a Diffuse that only feeds RowWiseNormalize / the Laplacian (no reference
   * equivalent; see sc_set_diffuse_mode): 0 = the handle's / process default, 1 = explicit fp64
   * product, 2 = matrix-free wherever the sequence allows it */
  int32_t diffuse_mode;
  int32_t reserved[4];
} sc_config;

typedef struct sc_diag {
  int32_t n;                     /* problem size */
  int32_t n_clusters_raw;        /* eigengap result before max(., min_clusters) */
  int32_t n_clusters;            /* value handed to k-means */
  int32_t eig_path;              /* SC_EIG_PATH_* */
  double max_delta;              /* max eigengap (utils.py:74-130, 2nd result) */
  int32_t n_eigenvalues;         /* entries valid in eigenvalues[] */
  int32_t eig_descending;        /* 1: largest first (None/Affinity); 0: smallest first */
  double eigenvalues[SC_MAX_EIG];/* in the order compute_sorted_eigenvectors returns */
  int32_t eig_matvec_passes;     /* passes over the n x n operator */
  int32_t eig_block;             /* vectors per pass */
  int32_t eig_basis;             /* Krylov basis size at exit */
  int32_t eig_cycles;            /* restart cycles used */
  double eig_max_residual;       /* max residual norm over accepted Ritz pairs */
  int32_t kmeans_iterations;     /* cosine k-means distance passes */
  int32_t symmetry_state;        /* 1 SYM, 2 DIAG*SYM (after RowWiseNormalize), 3 GENERAL */
  int32_t eig_host_chain;        /* 1: the fused Lanczos chain met a rank-deficient block and
                                    the host-driven repair chain redid the solve */
  int32_t eig_fallback;          /* 0, or why block Lanczos handed over to the dense path:
                                    1 restart budget spent, 2 projected eigenproblem failed,
                                    3 no full-rank Krylov block, 4 forced (SC_EIG_FORCE_DENSE),
                                    5 more than 64 eigenvectors wanted (> 64 selected clusters),
                                    7 eight equal Ritz values ahead of the decisive gap (an
                                    eigenvalue of multiplicity > 8: the dense path counts it);
                                    on the general path (eig_path 7) also 6: every eigenvalue
                                    is read (max_clusters=None with a Laplacian), 8: n <= 512,
                                    where the dense route is the default, 9: ascending
                                    NormalizedDiff reads np.max(eigenvalues), the far end of
                                    the spectrum (utils.py:110,123) */
  float stage_ms[SC_MAX_STAGES]; /* hipEvent time per SC_STAGE_* slot */
  int32_t diffuse_path;          /* SC_DIFFUSE_PATH_* */
  int32_t free_candidates;       /* matrix-free Diffuse: exact dot products evaluated (n + few) */
  int32_t free_overflow_rows;    /* ... rows evaluated in full (more candidates than the cap) */
  int32_t free_tiles_run;        /* ... 128 x 128 tiles of the digit product that were computed:
                                    the others -- of ceil(n/128) (ceil(n/128) + 1) / 2 -- were
                                    excluded by the segment-norm bound */
} sc_diag;

/* ---- library / device ---------------------------------------------------- */
int sc_abi_version(void);
/* sizeof(sc_config) / sizeof(sc_diag) as compiled, so a binding can verify its mirror */
int sc_struct_sizes(int* config_bytes, int* diag_bytes);

/* ---- described arrays (additions to ABI 7) --------------------------------
 * Where the embeddings are and what they look like.  The library reads them in place: a
 * device array by a kernel of its own (any element strides; 16-byte loads when col_stride is 1
 * and the base address and the row pitch in bytes are multiples of 16), a host array of a
 * narrow dtype by a copy at its own width into a staging buffer of the handle and the same
 * kernel.  All arithmetic stays fp64: widening fp32 / fp16 / bf16 is exact for every bit
 * pattern (subnormals, +-0, +-inf; a NaN stays a NaN), so every result is bit for bit what the
 * caller would get from the values converted to double on the host. */
enum {
  SC_DTYPE_F64 = 0, SC_DTYPE_F32 = 1, SC_DTYPE_F16 = 2, SC_DTYPE_BF16 = 3,
  /* label arrays only (sc_cluster_centroids_arrays, sc_labels_egress): every other entry answers
   * them as it answers any dtype it does not know, SC_ERR_INVALID "unknown dtype" */
  SC_DTYPE_I64 = 4, SC_DTYPE_I32 = 5
};
enum { SC_MEM_HOST = 0, SC_MEM_DEVICE = 1 };
typedef struct sc_array {
  const void* data;    /* first element (a byte offset of the owner already applied) */
  int32_t dtype;       /* SC_DTYPE_* */
  int32_t location;    /* SC_MEM_HOST: pageable or pinned host memory; SC_MEM_DEVICE: memory of
                          the handle's device */
  int64_t rows, cols;  /* (n, d) */
  int64_t row_stride;  /* elements (not bytes) from one row to the next, >= 0 */
  int64_t col_stride;  /* elements from one column to the next, >= 0 (1: rows are contiguous) */
} sc_array;
/* sizeof(sc_array) and the byte offsets of its seven fields in declaration order, as compiled
 * (a binding checks its mirror; sc_struct_sizes keeps its signature) */
int sc_array_layout(int* array_bytes, int* field_offsets);
/* number of visible HIP devices (0 if none / runtime unavailable) */
int sc_device_count(void);
/* copies the device name (e.g. "AMD Instinct MI355X") and gcnArchName */
int sc_device_info(int device, char* name, int name_len, char* arch, int arch_len,
                   int* compute_units, int64_t* total_mem_bytes);

/* ---- handle -------------------------------------------------------------- */
int sc_create(int device, sc_handle* out);
int sc_destroy(sc_handle h);
/* pre-size the device arena for problems up to (n_max, d_max); optional */
int sc_reserve(sc_handle h, int n_max, int d_max);
const char* sc_last_error(sc_handle h);
int sc_synchronize(sc_handle h);
/* The handle's hipStream_t.  Every *_array call reads a device source on this stream (a batch:
 * after one synchronisation of it, see sc_predict_batch_arrays), so a producer orders its
 * writes before the call by making this stream wait for them -- the `stream` argument of
 * __dlpack__ does exactly that.  NULL for a NULL handle. */
void* sc_stream(sc_handle h);
/* hipEvent timers in sc_diag.stage_ms: 1 (default) = one pair per stage, 2 = additionally
 * around the individual hot kernels (bench.py's per-kernel roofline list) */
int sc_set_profiling(sc_handle h, int level);
/* Route of a Diffuse (refinement.py:229-234) that is followed only by RowWiseNormalize and the
 * Laplacian -- the ICASSP2018 sequence.  0 (default): matrix-free from n = 2048 on (S = A A^T is
 * never formed: rowmax(S) from an exact 8-bit-digit integer MFMA product + fp64 recheck of the
 * candidates within a proven slack, the eigensolver applies A twice); 1: always the explicit
 * fp64 MFMA product; 2: matrix-free wherever the sequence allows it (n > 128); -1: back to
 * the process default (environment SC_DIFFUSE=explicit|free|auto, SC_DIFFUSE_FREE_MIN_N).
 * Both routes return the same rowmax / rowsum to summation order; sc_diag.diffuse_path says
 * which one ran. */
int sc_set_diffuse_mode(sc_handle h, int mode);
/* Tile skip list of the matrix-free route's digit product (ABI 7): 1 (default) = tiles that a
 * Cauchy-Schwarz bound on 64-column digit-segment norms proves free of row maxima and candidates
 * are not computed (exact for any input: rowmax / rowsum / candidate sets are those of the full
 * product); 0 = every tile (A/B measurements, parity tests); -1 = the process default
 * (environment SC_FREE_NO_PRUNE).  sc_diag.free_tiles_run reports what ran. */
int sc_set_free_prune(sc_handle h, int on);

/* fills cfg with the reference defaults (refinement.py:76-100,
 * spectral_clusterer.py:29-46): no ops, sigma 1 weights, p .95, mult .01 ... */
int sc_config_default(sc_config* cfg);
/* scipy.ndimage _gaussian_kernel1d(sigma, order 0, radius int(4 sigma + .5)) */
int sc_gaussian_weights(double sigma, int32_t* radius, double* weights);
/* GaussianBlur with sigma > 8 (radius > SC_MAX_BLUR_RADIUS; refinement.py:154-162 has no
 * limit): its 2 * radius + 1 weights do not fit sc_config -- upload them once, they stay
 * resident in the handle, and a config with blur_radius == radius uses them.  Such a config
 * carries the CENTRAL 2 * SC_MAX_BLUR_RADIUS + 1 weights (weights[radius - 32 .. radius + 32])
 * in cfg->blur_weights: every call checks them against the resident ones, so two sigmas that
 * share a radius cannot be confused (SC_ERR_UNSUPPORTED: upload again). */
int sc_set_blur_weights(sc_handle h, int radius, const double* weights);

/* ---- whole path ---------------------------------------------------------- */
/*
 * SpectralClusterer.predict (spectral_clusterer.py:201-314) for the in-scope
 * branch: affinity -> refinement -> Laplacian -> top-k eigen + eigengap ->
 * cosine k-means.  X: (n, d).  labels: n int64 (caller-allocated).
 */
int sc_predict(sc_handle h, const double* x, int n, int d, const sc_config* cfg,
               int64_t* labels, sc_diag* diag);

/* sc_predict on a described source (device or host, fp64 / fp32 / fp16 / bf16, any strides).
 * SC_ERR_INVALID before any launch for: NULL data, rows or cols <= 0, an unknown dtype or
 * location, a negative stride, and a SC_MEM_DEVICE pointer that hipPointerGetAttributes does not
 * report as device memory of the handle's device.  sc_predict(h, x, n, d, ...) is this call on
 * {x, SC_DTYPE_F64, SC_MEM_HOST, n, d, d, 1}. */
int sc_predict_array(sc_handle h, const sc_array* x, const sc_config* cfg, int64_t* labels,
                     sc_diag* diag);

/* Split form, used for device-resident timing and by AutoTune:            */
/* H2D of the embeddings into the handle's arena. */
int sc_set_embeddings(sc_handle h, const double* x, int n, int d);
/* ... of a described source.  Like sc_set_embeddings it returns with the handle's stream
 * synchronised: the source may be overwritten or freed at once. */
int sc_set_embeddings_array(sc_handle h, const sc_array* x);
/* utils.compute_affinity_matrix (utils.py:20-41) on the resident embeddings. */
int sc_compute_affinity(sc_handle h);
/* H2D of a caller-supplied (n, n) affinity (custom affinity_function /
 * _compute_eigenvectors_ncluster(affinity), spectral_clusterer.py:108). */
int sc_set_affinity(sc_handle h, const double* affinity, int n);
/* ... of a described (n, n) source, read where it is: device or host memory, fp64 / fp32 / fp16 /
 * bf16, any non-negative element strides (a transposed view, a [::2, ::2] slice).  It is widened
 * exactly on the device, so the resident affinity is bit for bit the source converted to double
 * on the host; the padding columns n .. ld of the resident rows are zero.  A device source and a
 * narrow host source are widened by one kernel that decides the exact symmetry of the matrix in
 * the same pass; a host fp64 source goes up by a 2-D copy as in sc_set_affinity.  The handle's
 * state afterwards is that of sc_set_affinity.  SC_ERR_INVALID before any launch for what
 * sc_predict_array rejects and for rows != cols.  Returns with the handle's stream synchronised:
 * the source may be overwritten or freed at once. */
int sc_set_affinity_array(sc_handle h, const sc_array* affinity);
/* predict() from an affinity the caller holds: sc_set_affinity_array, the before-refinement
 * constraint if one is resident, sc_eig_ncluster, sc_cluster -- sc_predict_array without the
 * embeddings and the affinity GEMM.  diag->stage_ms[SC_STAGE_AFFINITY] is the constraint's time
 * (the ingest is host-synchronous: time it on the host). */
int sc_predict_affinity_array(sc_handle h, const sc_array* affinity, const sc_config* cfg,
                              int64_t* labels, sc_diag* diag);
/*
 * SpectralClusterer._compute_eigenvectors_ncluster (spectral_clusterer.py:
 * 108-168) on the resident affinity, which is left untouched (AutoTune calls
 * this once per p_percentile, spectral_clusterer.py:274-287).  Eigenvectors
 * stay on the device; diag receives eigenvalues, n_clusters_raw, max_delta.
 */
int sc_eig_ncluster(sc_handle h, const sc_config* cfg, sc_diag* diag);
/* The eigenvalues the last sc_eig_ncluster / sc_predict consumed, in the order
 * compute_sorted_eigenvectors returns them (utils.py:62-70): sc_diag.eigenvalues holds at
 * most SC_MAX_EIG of them, these calls give all (n of them with max_clusters=None). */
int sc_num_eigenvalues(sc_handle h);
int sc_get_eigenvalues(sc_handle h, double* out, int count);
/* number of eigenvector columns currently resident */
int sc_num_eigenvectors(sc_handle h);
/* D2H of the first ncols resident eigenvectors as an (n, ncols) matrix */
int sc_get_eigenvectors(sc_handle h, double* out, int n, int ncols);
/*
 * predict() tail (spectral_clusterer.py:295-313): slice [:, :n_clusters],
 * optional row re-norm, run_kmeans (custom_distance_kmeans.py:13-52).
 */
int sc_cluster(sc_handle h, const sc_config* cfg, int n_clusters,
               int64_t* labels, sc_diag* diag);
/*
 * Constraints (constraint.py:95-164; spectral_clusterer.py:137-142, 259-264).
 * sc_set_constraint uploads the (n, n) constraint matrix (it stays resident until
 * sc_clear_constraint; exact symmetry is detected on the device).  While one is
 * resident and cfg->constraint_name != 0:
 *   - apply_before_refinement: sc_predict / sc_run_resident adjust the affinity right
 *     after computing it; on the split path call sc_apply_constraint once after
 *     sc_compute_affinity / sc_set_affinity (it rewrites the resident affinity);
 *   - otherwise sc_eig_ncluster adjusts the refined matrix (each call).
 * ConstraintPropagation's (I - alpha A_norm)^-1 is evaluated as the Neumann product
 * prod_j (I + (alpha A_norm)^(2^j)) with fp64 MFMA GEMMs, which needs |alpha| < 1 and
 * a non-negative affinity (spectral radius of A_norm <= 1) -- both hold for the
 * reference's cosine affinity and its 0.4 / 0.6 presets.
 *
 * The banded form.  ConstraintMatrix.compute_diagonals (constraint.py:188-201) builds an
 * (n, n) matrix whose only non-zeros sit on the first super- and sub-diagonal;
 * sc_set_constraint_band takes those n - 1 values instead: band[i] = Q[i, i+1] = Q[i+1, i],
 * every other entry of Q (the diagonal included) is 0.  n - 1 doubles are uploaded (n = 1:
 * none, band may be NULL); no (n, n) buffer, no symmetry kernel.  The two forms replace one
 * another, sc_clear_constraint clears either, and everything above holds for both: a band
 * behaves as the symmetric dense matrix it stands for.  AffinityIntegration reads band[min(i,
 * j)] where |i - j| == 1; ConstraintPropagation forms T Q in one pass over T (two terms per
 * entry) instead of an n^3 GEMM.
 * sc_constraint_info reports the resident form -- kind 0 none / 1 dense / 2 band, its n (0 when
 * none) -- and the current device sizes in bytes of the band buffer and of the (n, ld) dense
 * buffer (buffers are kept across calls; one that was never needed stays 0).  Any out pointer
 * may be NULL.
 *
 * The entry-list form: a handful of must-link / cannot-link pairs, what E2CP is about.
 * sc_set_constraint_pairs takes Q as its `count` non-zero entries Q[rows[e], cols[e]] = vals[e]
 * (host memory; a symmetric pair is two entries).  count * 16 bytes are uploaded, nothing else;
 * count = 0 is valid (Q = 0).  SC_ERR_INVALID: an index outside [0, n), a non-finite value, a
 * position listed twice.  Whether the list is symmetric -- every (r, c, v) with r != c has its
 * twin (c, r, v) -- is decided on the host while validating; an asymmetric list behaves as the
 * asymmetric dense matrix it stands for.  It replaces a dense or banded constraint and is
 * replaced by them, sc_clear_constraint clears it, sc_constraint_info reports kind 3, and
 * sc_constraint_pairs_info the entry count (0 when another form or none is resident) and the
 * current device size in bytes of the entry buffer.
 * AffinityIntegration: one pass over A with Q = 0, then the `count` entries are patched from the
 * originals gathered before it.  ConstraintPropagation, count <= n: T Q T = sum_e vals[e]
 * T[:, rows[e]] T[cols[e], :] = U V^T with two (n, round_up(count, 16)) panels held in idle work
 * matrices; one kernel forms U V^T tile by tile (fp64 MFMA, entry order, no atomics) and adjusts
 * A with it in registers -- instead of two n^3 GEMMs and three more passes.  count > n: the
 * entries are scattered into the zero-filled dense buffer on the device and the dense stage
 * runs (still no (n, n) upload).  When A and the list are symmetric the result is exactly
 * symmetric.
 */
int sc_set_constraint(sc_handle h, const double* constraint_matrix, int n);
/* constraint.py:167-207 (ConstraintMatrix) + sc_set_constraint, without the matrix */
int sc_set_constraint_band(sc_handle h, const double* band, int n);
/* sc_set_constraint with the matrix given as its non-zero entries */
int sc_set_constraint_pairs(sc_handle h, const int32_t* rows, const int32_t* cols,
                            const double* vals, int count, int n);
int sc_constraint_pairs_info(sc_handle h, int* count, size_t* pair_bytes);
/* sc_set_constraint for a described (n, n) source, read where it is: device or host memory, fp64 /
 * fp32 / fp16 / bf16, any non-negative element strides (sc_set_affinity_array's rules and errors).
 * A device source is read in place, a narrow host source crosses the link at its own width; the
 * kernel that widens it (exactly) into the resident matrix decides its symmetry in the same pass
 * (a host fp64 source takes sc_set_constraint's copy and separate pass).  The source may be
 * reused when the call has returned.  State afterwards is sc_set_constraint's: sc_constraint_info
 * kind 1.  The dense arithmetic runs whatever the matrix holds: no structure is detected. */
int sc_set_constraint_array(sc_handle h, const sc_array* constraint_matrix);
int sc_clear_constraint(sc_handle h);
int sc_apply_constraint(sc_handle h, const sc_config* cfg);
int sc_constraint_info(sc_handle h, int* kind, int* n, size_t* band_bytes,
                       size_t* dense_bytes);
/* affinity + eig_ncluster + cluster on the resident embeddings (no H2D of X) */
int sc_run_resident(sc_handle h, const sc_config* cfg, int64_t* labels,
                    sc_diag* diag);
/* one AutoTune search level (autotune.py:98-111): sc_eig_ncluster for `count` values of
 * p_percentile on the resident affinity; diags[i] reports what sc_eig_ncluster would for
 * p_values[i].  The values of a level differ only in the row threshold: the stages after it
 * run as grouped launches, the eigensolvers in lockstep.  At n <= 128 the values are
 * (matrix, p) pairs: one front launch and ONE dense Jacobi launch, a workgroup per value, for up
 * to 64 of them (the two sequences the larger sizes group; anything else one by one).  Leaves no
 * eigenvectors resident in the handle itself (sc_sweep_adopt fetches a value's). */
int sc_eig_ncluster_sweep(sc_handle h, const sc_config* cfg, const double* p_values, int count,
                          sc_diag* diags);
/* The eigenvectors of value `index` of the last sweep become the resident ones -- what
 * sc_eig_ncluster with p_values[index] would leave, without evaluating the winner a second
 * time (the reference's search keeps the winner's eigenvectors, spectral_clusterer.py:
 * 274-292).  cfg: the sweep's configuration with p_percentile = p_values[index] (checked).
 * SC_ERR_UNSUPPORTED when that value's solve left the grouped path or the configuration is
 * not the sweep's (then call sc_eig_ncluster).  Follow with sc_cluster. */
int sc_sweep_adopt(sc_handle h, const sc_config* cfg, int index, sc_diag* diag);
/* a Python `for` over predict() in the reference: count
 * independent utterances, xs[i] is (ns[i], d); labels[i] has ns[i] slots. */
int sc_predict_batch(sc_handle h, const double* const* xs, const int* ns, int d,
                     int count, const sc_config* cfg, int64_t* const* labels,
                     sc_diag* diags);
/* the same over `streams` HIP streams of the handle's device (pooled arenas, one host
 * thread per stream inside the call, longest utterances first): small utterances cannot
 * fill the GPU and their pipeline is latency-bound, several in flight overlap */
int sc_predict_batch_streams(sc_handle h, const double* const* xs, const int* ns, int d,
                             int count, const sc_config* cfg, int64_t* const* labels,
                             sc_diag* diags, int streams);
/* the same as groups of `group` (<= 16) utterances per launch: the stages before the
 * eigensolver are enqueued member after member (one launch for all members' GEMM tiles when
 * the sequence is the ICASSP2018 one), the block Lanczos chain and the k-means chain of the
 * members advance in lockstep (one launch per step and one host synchronisation per check for
 * the whole group).  The groups are dealt to up to three lanes -- internal lead handles with
 * their own streams, member arenas and host thread -- so up to three groups' chains are in
 * flight; the call returns when all lanes are done.  Per-utterance results agree with
 * sc_predict to the solver's tolerance (whole-K tile sums where a short single call splits
 * K; the group's check schedule), not bit for bit; the same batch always gives the same
 * results.  That is the route of 128 < n < 4096.  Utterances of n <= 128 take the short
 * route: the dense Jacobi eigensolver of the single call with one workgroup per utterance,
 * up to 64 utterances per launch and one synchronisation per launch, then the same lockstep
 * k-means; the kernel body, its arguments and the LDS layout are sc_predict's (eigenvalues
 * within 1e-10 relative of it, equal labels), full-spectrum requests included.  Everything
 * else (n >= 4096, a full-spectrum request above 128, non-cosine k-means, constraints -- a
 * resident constraint with a configured operator: this entry carries one for the whole batch or
 * none; sc_predict_batch_constrained carries one band per utterance through the grouped routes --,
 * group < 2) and every member that leaves its route (a refinement that is not symmetric,
 * more than 32 clusters, a rare branch of the eigensolver) takes the single-call path.
 * sc_last_batch_routes says what ran. */
int sc_predict_batch_grouped(sc_handle h, const double* const* xs, const int* ns, int d,
                             int count, const sc_config* cfg, int64_t* const* labels,
                             sc_diag* diags, int group);
/* A batch of described sources (all with the same cols): group > 1 is sc_predict_batch_grouped
 * with that group size, anything else sc_predict_batch_streams with `streams`.  Every
 * descriptor is validated before the first launch.  When a source is SC_MEM_DEVICE the call
 * synchronises the handle's stream ONCE at entry; after that the member streams, lanes and
 * banks of the batch read the sources freely -- so work that the caller ordered before
 * sc_stream(h) is complete before anything of the batch reads it.  The upload that rides under
 * the previous call's pipeline (sc_predict_batch) is for host fp64 sources; device sources are
 * widened by a kernel on the call's own stream, narrow host sources are copied per call. */
int sc_predict_batch_arrays(sc_handle h, const sc_array* xs, int count, const sc_config* cfg,
                            int64_t* const* labels, sc_diag* diags, int group, int streams);
/* sc_predict_batch_arrays in its grouped form (group >= 2, else SC_ERR_INVALID) with speaker-turn
 * constraints: bands[i] is the band of utterance i's ConstraintMatrix (constraint.py:167-207;
 * xs[i].rows - 1 values as sc_set_constraint_band takes them, host memory, valid for the call), or
 * NULL for an utterance without a constraint; bands == NULL: none has one.  The operator and its
 * position come from cfg (constraint_name NONE: the bands are not read).  Routes, groups, banks and
 * short waves are those of sc_predict_batch_grouped, on one lane with member-by-member fronts:
 * each member's band becomes the resident constraint of its member arena.  ConstraintPropagation
 * before refinement runs as ONE chain of grouped launches per group (up to 16 members per launch,
 * a short wave of 64 in four chunks): the Neumann products of all members share a launch, each tile
 * with its whole K.  AffinityIntegration, and ConstraintPropagation after refinement, run per
 * member as in sc_predict.  Members without a band are idle in the chain and otherwise unchanged.
 * The chain's work matrices are reserved with the member arenas before the first front; when
 * hipMemGetInfo says they do not fit, the members that carry a band run as single calls (route 0).
 * The resident constraint of h itself is not read; none is resident in h or in any member arena
 * when the call returns, whatever it returns.  Every descriptor is validated before the first
 * launch.  A band of the wrong length cannot be detected here. */
int sc_predict_batch_constrained(sc_handle h, const sc_array* xs, const double* const* bands,
                                 int count, const sc_config* cfg, int64_t* const* labels,
                                 sc_diag* diags, int group);
/* The constraint of one utterance of sc_predict_batch_constraints; every pointer is host memory,
 * valid for the duration of the call.  kind: sc_constraint_info's codes -- 0 none, 2 band (`band`:
 * rows - 1 values), 3 pairs (`count` directed entries rows / cols / vals as
 * sc_set_constraint_pairs takes them); the fields of the other kinds are not read. */
typedef struct sc_constraint_desc {
  int32_t kind;
  int32_t count;
  const double* band;
  const int32_t* rows;
  const int32_t* cols;
  const double* vals;
} sc_constraint_desc;
/* sizeof(sc_constraint_desc) and the offsets of its 6 fields in declaration order (either may be
 * NULL): lets a binding check its mirror of the struct, as sc_array_layout does */
int sc_constraint_desc_layout(int* bytes, int* field_offsets);
/* sc_predict_batch_constrained with one sc_constraint_desc per utterance (cons == NULL: none has a
 * constraint); that function is this one with every kind 0 or 2.  An entry list becomes the
 * resident constraint (kind 3) of its member arena, behind the affinity, in buffers reserved with
 * the arena for the batch's largest list.  In ConstraintPropagation before refinement the Neumann
 * chain is shared by all members of a group; its last stage runs the band members' three launches
 * with the pair members idle, then the pair members' two (k_cp_pair_panels_g,
 * k_cp_pairs_adjust_g) with the band members idle; a launch without live members is skipped.  A
 * member with more entries than rows takes the dense stage and runs as a single call (route 0).
 * Every list is validated before the first launch (SC_ERR_INVALID as sc_set_constraint_pairs). */
int sc_predict_batch_constraints(sc_handle h, const sc_array* xs, const sc_constraint_desc* cons,
                                 int count, const sc_config* cfg, int64_t* const* labels,
                                 sc_diag* diags, int group);
/* [predict_affinity(a_i, c_i)]: sc_predict_batch_constraints for (n_i, n_i) affinities the caller
 * holds (sc_set_affinity_array's sources, any mix of dtypes, layouts and locations) instead of
 * embeddings; cons may be NULL.  The same routes (sc_last_batch_routes): n <= 128 in Jacobi waves
 * of up to 64, 128 < n < 4096 as lockstep groups of up to `group`, the rest and members that leave
 * their route as single calls inside the call.  A group or wave is ingested by ONE
 * k_ingest_affinity_group launch, and the host reads its members' symmetry flags in one wait;
 * the members then take the member-by-member front (the fused fronts read CropDiagonal's value
 * and a cosine bound from the affinity GEMM's epilogue).  A member that is not symmetric and
 * whose sequence does not symmetrise it leaves its route for the general solver.  With a device
 * source the handle's stream is synchronised once at entry; sources stay valid until return. */
int sc_predict_batch_affinities(sc_handle h, const sc_array* affinities,
                                const sc_constraint_desc* cons, int count, const sc_config* cfg,
                                int64_t* const* labels, sc_diag* diags, int group);
/* sc_predict_batch_constraints (affinities = 0: xs are embeddings) or sc_predict_batch_affinities
 * (affinities != 0: xs are (n_i, n_i) affinities) plus a parallel list `dense` of dense constraint
 * matrices as described sources (sc_set_constraint_array's: device or host, four dtypes, strides).
 * dense[i].data != NULL: utterance i carries the (n_i, n_i) matrix dense[i], and cons[i].kind must
 * be 0; otherwise cons[i] applies as in those calls.  cons or dense may be NULL; with dense == NULL
 * the call is exactly the existing one.  Dense members travel the same routes.  The dense sources of
 * a group or wave are widened into their member arenas' constraint buffers by k_ingest_affinity_group
 * launches (one per <= 64 sources) and the host reads their symmetry flags in one wait (the wait of
 * the affinities' ingest, where there is one).  In ConstraintPropagation before refinement a member
 * with a symmetric affinity and a symmetric dense constraint joins the group's Neumann chain, whose
 * last stage runs the dense members' three launches (T Q^T by the full-output grouped product,
 * T (T Q^T)^T by the symmetric one, the adjustment) with the band and pair members idle; any other
 * dense member runs its own operator on its arena (sc_apply_constraint).  The member arenas reserve
 * one more n x ld matrix each; when that does not fit, the constrained members run as single calls
 * (route 0), a dense one with sc_set_constraint_array in front -- as every dense member of
 * n >= 4096 does.  Every source and every entry list is validated before the first launch.  With a
 * device source the handle's stream is synchronised once at entry; sources stay valid until return. */
int sc_predict_batch_constraint_arrays(sc_handle h, const sc_array* xs,
                                       const sc_constraint_desc* cons, const sc_array* dense,
                                       int count, const sc_config* cfg, int64_t* const* labels,
                                       sc_diag* diags, int group, int affinities);
/* What ran: one code per utterance of the last sc_predict_batch* call on this handle (a
 * member of a grouped batch that was handed back to the single-call path reports
 * SC_BATCH_ROUTE_SINGLE; after sc_predict_batch / sc_predict_batch_streams every code is).
 * SC_ERR_INVALID for a NULL handle, NULL `routes`, or a `count` that is not the last batch's. */
enum {
  SC_BATCH_ROUTE_SINGLE = 0,         /* the single-call path, on the member's arena */
  SC_BATCH_ROUTE_GROUP_LANCZOS = 1,  /* lockstep block Lanczos of a group (128 < n < 4096) */
  SC_BATCH_ROUTE_GROUP_JACOBI = 2,   /* short route: one Jacobi workgroup per member (n <= 128) */
  SC_BATCH_ROUTE_FALLBACK = 3        /* sc_predict_batch_reduced: the agglomerative fallback;
                                        sc_predict_batch_single_fallback: found single */
};
int sc_last_batch_routes(sc_handle h, int32_t* routes, int count);
/* A per-handle permission (default off).  Off: the grouped and short routes of every batch call
 * take cfg->kmeans_metric == SC_KMEANS_COSINE alone, and an utterance under any other metric runs
 * as a single call inside the batch call (route 0), whose k-means is the single-workgroup kernel.
 * On: every SC_KMEANS_* metric takes the routes cosine takes, in every batch call that ends in
 * the grouped batch (plain, constrained, affinities, single, single_fallback / _naive, reduced /
 * _naive, multi_stage); its k-means is the lockstep chain with the metric's distance in the
 * assignment.  Labels then equal the single call's unless an assignment or the stop rule is a
 * near tie (the two kernels add in different orders).  sc_predict_batch_autotune and the stream
 * pool do not read it.  The caller sets it before a batch call and clears it afterwards; it
 * changes nothing else.  SC_ERR_INVALID for a NULL handle. */
int sc_set_batch_any_metric(sc_handle h, int on);

/*
 * Size reduction before the spectral path (spectral_clusterer.py:170-199,
 * multi_stage_clusterer.py:109-112, fallback_clusterer.py:108-113):
 * sklearn.cluster.AgglomerativeClustering(metric="cosine", linkage=...).fit_predict(X)
 * with n_clusters > 0, or n_clusters == 0 and a distance_threshold; labels are numbered as
 * sklearn numbers them.  n_clusters_out (may be NULL) receives the cluster count.
 */
int sc_ahc(sc_handle h, const double* x, int n, int d, int linkage, int n_clusters,
           double distance_threshold, int64_t* labels, int* n_clusters_out);
/* utils.get_cluster_centroids (utils.py:159-176): out is (k, d), k = max(labels) + 1 */
int sc_cluster_centroids(sc_handle h, const double* x, int n, int d, const int64_t* labels,
                         int k, double* out);
/* sc_ahc for every listed array (any dtype, host or device memory, the same cols; each at least
 * 2 rows) in one call, and optionally utils.get_cluster_centroids of each: centroids (may be NULL,
 * or hold NULL entries) receives (k_i, cols) doubles, k_i = n_clusters, or at most rows_i when
 * the tree is cut at distance_threshold.  Every descriptor is validated before the first launch.
 * The call works in waves: the longest remaining members whose buffers fit the wave budget share
 * one allocation, one launch per step (a workgroup per member in the chain, a wavefront per member
 * of up to 128 rows under average linkage) and ONE synchronisation before their trees are cut on
 * host threads.  A member that alone exceeds the budget, or has 4096 rows or more, runs sc_ahc's
 * own path inside the call.  A member with a zero or non-finite row fails the call with
 * SC_ERR_INVALID; the message names its index. */
int sc_batch_ahc(sc_handle h, const sc_array* xs, int count, int linkage, int n_clusters,
                 double distance_threshold, int64_t* const* labels, double* const* centroids);
/* Bytes of device memory a wave of sc_batch_ahc / sc_predict_batch_reduced may take; 0 (the
 * default): half of what hipMemGetInfo reports free when the wave is planned. */
int sc_set_reduce_wave_bytes(sc_handle h, size_t bytes);
/* sc_predict_batch_arrays in its grouped form for a clusterer with max_spectral_size and / or
 * fallback_options.spectral_min_embeddings (spectral_clusterer.py:170-199, 229-248;
 * fallback_clusterer.py:108-124).  Utterance i is of kind
 *   2  rows < spectral_min_embeddings: average-linkage AHC cut at agglomerative_threshold,
 *   1  max_spectral_size > 0 and rows > max_spectral_size: complete-linkage AHC down to
 *      max_spectral_size clusters, the spectral path on their centroids (which stay on the
 *      device), labels[i][r] = spectral label of row r's cluster,
 *   0  everything else: the spectral path on the rows.
 * Kinds 1 and 2 run as sc_batch_ahc runs them; then ONE grouped batch clusters the rows of kind 0
 * and the centroids of kind 1.  diags[i] is the spectral run's (zeroed for kind 2),
 * sc_last_batch_routes reports its route, SC_BATCH_ROUTE_FALLBACK for kind 2.  kinds (may be
 * NULL) receives the kind of every utterance. */
int sc_predict_batch_reduced(sc_handle h, const sc_array* xs, int count, const sc_config* cfg,
                             int max_spectral_size, int spectral_min_embeddings,
                             double agglomerative_threshold, int64_t* const* labels,
                             sc_diag* diags, int group, int32_t* kinds);

/*
 * min_clusters = 1: the single-cluster test (fallback_clusterer.py:127-187) inside the batch.
 * `condition` is one of the four conditions that read the affinity (the values of
 * SingleClusterCondition); the FallbackClusterer condition reads the embeddings, not the
 * affinity: its batched form is sc_predict_batch_single_fallback below, which takes no
 * sc_single_check.  diagonal_offset is read by SC_SINGLE_GMM_BIC alone, threshold by the other
 * three.
 */
enum {
  SC_SINGLE_GMM_BIC = 1,           /* bic1 < bic2 of sc_affinity_gmm_bic */
  SC_SINGLE_ALL_AFFINITY = 2,      /* affinity.min() > threshold */
  SC_SINGLE_NEIGHBOR_AFFINITY = 3, /* np.diag(affinity, 1).min() > threshold */
  SC_SINGLE_AFFINITY_STD = 4       /* np.std(affinity) < threshold */
};
typedef struct sc_single_check {
  int32_t condition;        /* SingleClusterCondition: 1 GmmBic, 2 All, 3 Neighbor, 4 Std */
  int32_t diagonal_offset;
  double  threshold;
} sc_single_check;
/* sizeof(sc_single_check) and the byte offsets of its 3 fields, in declaration order (a binding
 * checks its mirror against them) */
int sc_single_check_layout(int* check_bytes, int* field_offsets);
/* sc_predict_batch_arrays in its grouped form (group >= 2, else SC_ERR_INVALID) for a clusterer
 * with min_clusters = 1: every utterance's raw affinity is tested before its eigensolver runs, and
 * an utterance found to hold one cluster gets labels of zeros, a zeroed diag and single[i] = 1 (0
 * otherwise; single may be NULL).  The test is group-wide device work on the routes of the batch
 * (sc_last_batch_routes reports the route the utterance's affinity took): n <= 128, ONE launch
 * per wave of up to 64 utterances, a workgroup each, the whole decision in the kernel; 128 < n <
 * 4096, launches over (row blocks x members) for a group of up to 16, parameters updated on the
 * device, one look at the members' state per 8 launches; n >= 4096 and whatever else takes route
 * 0, sc_affinity_stats / sc_affinity_gmm_bic's own code on the handle.  The refinement front of
 * an utterance has been enqueued before its verdict is known; a single-cluster utterance leaves
 * before the eigensolver.  Arithmetic, start, stop rules and constants are those of
 * sc_affinity_stats / sc_affinity_gmm_bic; the sums are taken in another (fixed) order, so the
 * BICs agree to rounding (1e-9 relative), the minima bit for bit.  check == NULL:
 * sc_predict_batch_arrays.  With SC_SINGLE_GMM_BIC an utterance of diagonal_offset >= rows - 1
 * (or a negative offset) fails the call with SC_ERR_INVALID before anything is launched:
 * sc_affinity_gmm_bic's message and "(utterance i)". */
int sc_predict_batch_single(sc_handle h, const sc_array* xs, int count, const sc_config* cfg,
                            const sc_single_check* check, int64_t* const* labels,
                            sc_diag* diags, int group, int32_t* single);
/* The decision alone, on `count` affinity matrices in host memory (affinities[i]: ns[i] x ns[i]
 * row-major doubles), through exactly the kernels the batch runs (the short form for n <= 128,
 * the chain form for 128 < n < 4096; n >= 4096: the single call's): values = count x 8 doubles
 * {min, neighbour min, mean, std, bic1, bic2, lloyd steps, em steps} -- the last four are 0
 * unless the condition is SC_SINGLE_GMM_BIC; lloyd steps / em steps: passes of the Lloyd loop /
 * of the EM loop of the 2-component fit --, single[i] = 1 for one cluster.  A matrix's values do
 * not depend on what else is in the call.  Every argument is checked before the first launch
 * (diagonal_offset as above): values and single are untouched then. */
int sc_batch_single_check(sc_handle h, const double* const* affinities, const int* ns, int count,
                          const sc_single_check* check, double* values, int32_t* single);

/*
 * min_clusters = 1 with the FallbackClusterer condition and the agglomerative fallback type
 * (fallback_clusterer.py:108-124, 174-176; what MultiStageClusterer's constructor sets): an
 * utterance holds one cluster when average-linkage cosine AHC, cut at distance_threshold, leaves
 * one -- when no merge height is >= distance_threshold.
 *
 * sc_batch_fallback_check: the decision alone, through exactly the kernels the batch runs.  The
 * arrays are sc_batch_ahc's (any dtype, host or device memory, the same cols, at least 2 rows
 * each), taken in its waves (sc_set_reduce_wave_bytes) with its distances (unit rows, the grouped
 * fp64 product, 1 - clip), then the VERDICT forms of its two linkage kernels: a wavefront per
 * member of up to 128 rows, a workgroup per longer member; no merge list is written, a wave
 * downloads one record per member.  single[i] = 1: one cluster, heights[i] the largest merge
 * height (sc_ahc's, bit for bit).  single[i] = 0: heights[i] is the first merge height found >=
 * distance_threshold, where the member's work ends.  A member's record does not depend on what
 * else is in the call.  A member of 4096 rows or more, or one that alone exceeds the wave budget,
 * runs sc_ahc's own path (heights[i] is then the largest height either way).  Every argument is
 * checked before the first launch; a member with a zero or non-finite row fails the call with
 * SC_ERR_INVALID and a message that names its index.  heights and single are written only when
 * the call succeeds.
 */
int sc_batch_fallback_check(sc_handle h, const sc_array* xs, int count,
                            double distance_threshold, double* heights, int32_t* single);
/* sc_predict_batch_arrays in its grouped form (group >= 2, else SC_ERR_INVALID) for such a
 * clusterer.  The verdicts of the WHOLE batch come first, as sc_batch_fallback_check computes
 * them; then ONE grouped batch clusters the utterances of several clusters.  An utterance found
 * single never enters the spectral path: labels of zeros, a zeroed diag, single[i] = 1 (0
 * otherwise; single may be NULL), route SC_BATCH_ROUTE_FALLBACK; the others report the route of
 * the grouped batch.  An utterance is ingested once: the widened fp64 rows of a wave stay on the
 * device and the grouped batch reads them there (ingest is exact), while the rows kept add up to
 * at most half a wave's budget; beyond that the grouped batch ingests the caller's array again.
 * An utterance of fewer than 2 rows fails the call with SC_ERR_INVALID before anything is
 * launched (sc_ahc's message and the utterance's index). */
int sc_predict_batch_single_fallback(sc_handle h, const sc_array* xs, int count,
                                     const sc_config* cfg, double distance_threshold,
                                     int64_t* const* labels, sc_diag* diags, int group,
                                     int32_t* single);

/*
 * The Naive fallback type (fallback_clusterer.py:114-118, naive_clusterer.py; what a default
 * FallbackOptions selects) for a whole batch: NaiveClusterer(threshold,
 * adaptation_threshold).predict from the EMPTY state for every listed array -- the first row
 * opens centroid 0; after that a cosine to every centroid, the first maximum wins, a new centroid
 * when best < threshold, a merge when best > adaptation_threshold.
 *
 * sc_batch_naive_cluster: the arrays may be of any dtype, in host or device memory, with the same
 * cols and at least 1 row each.  labels[i] receives rows_i labels, n_clusters[i] the number of
 * centroids.  centroids and counts may be NULL or hold NULL entries; centroids[i] holds rows_i x
 * cols doubles and counts[i] rows_i ints, of which the first n_clusters[i] rows / entries are
 * written.  Labels, counts and centroids are bit for bit those of sc_naive_cluster on the widened
 * fp64 rows with *n_centroids = 0 (both kernels share their arithmetic), for every input, zero
 * and NaN rows included.  The members are taken in sc_batch_ahc's waves
 * (sc_set_reduce_wave_bytes): the longest remaining members whose buffers fit the wave budget
 * share one allocation, one ingest per member, one table copy, ONE launch (a workgroup of 256
 * threads per member), one copy back and one synchronisation.  No size sends a member anywhere
 * else: one that alone exceeds the budget is a wave of its own.  Every argument is checked before
 * the first launch (SC_ERR_INVALID also for adaptation_threshold < threshold); the outputs are
 * written only when the call succeeds; a member's result does not depend on what else is in the
 * call.
 *
 * sc_batch_naive_check: "does the walk end with one centroid?" alone, through the VERDICT form of
 * the same kernel: a member's work ends at the row that would open a second centroid, no labels
 * or centroids are written, a wave downloads one record per member.  single[i] = 1 and
 * stopped_at[i] = rows_i when the walk ended with one centroid; otherwise single[i] = 0 and
 * stopped_at[i] is the index of the row that would open the second one (the first row
 * sc_batch_naive_cluster labels 1).  Zero and non-finite rows are walked as sc_naive_cluster
 * walks them; they fail nothing here.
 */
int sc_batch_naive_cluster(sc_handle h, const sc_array* xs, int count, double threshold,
                           double adaptation_threshold, int64_t* const* labels,
                           int32_t* n_clusters, double* const* centroids,
                           int32_t* const* counts);
int sc_batch_naive_check(sc_handle h, const sc_array* xs, int count, double threshold,
                         double adaptation_threshold, int32_t* single, int32_t* stopped_at);
/* sc_predict_batch_reduced with the Naive fallback type: the utterances of fewer than
 * spectral_min_embeddings rows (kind 2) are clustered by sc_batch_naive_cluster's waves inside the
 * call; one of a single row is fine (label 0).  Kinds 0 and 1, routes and diags are exactly
 * sc_predict_batch_reduced's (one body runs both calls). */
int sc_predict_batch_reduced_naive(sc_handle h, const sc_array* xs, int count,
                                   const sc_config* cfg, int max_spectral_size,
                                   int spectral_min_embeddings, double naive_threshold,
                                   double naive_adaptation_threshold, int64_t* const* labels,
                                   sc_diag* diags, int group, int32_t* kinds);
/* sc_predict_batch_single_fallback with the Naive fallback type: the verdicts are
 * sc_batch_naive_check's, and the widened rows of a wave stay on the device for the grouped batch
 * of the survivors under the same half-budget rule.  An utterance of one row is single (zeros,
 * route SC_BATCH_ROUTE_FALLBACK).  An utterance with a zero or non-finite row (the rule of the
 * unit-row kernel) fails the call with SC_ERR_INVALID and a message that names its index, whatever
 * its verdict, as the agglomerative form does. */
int sc_predict_batch_single_naive(sc_handle h, const sc_array* xs, int count,
                                  const sc_config* cfg, double naive_threshold,
                                  double naive_adaptation_threshold, int64_t* const* labels,
                                  sc_diag* diags, int group, int32_t* single);

/*
 * The multi-stage regime with min_clusters = 1 as one call: fallback_options.spectral_min_embeddings,
 * max_spectral_size and the single-cluster test together (spectral_clusterer.py:229-256, 170-199).
 * The three interact per utterance, so the calls above cannot be combined by partitioning a batch.
 */
/* SingleClusterCondition.FallbackClusterer: a value of sc_multi_stage.single_condition only (an
 * sc_single_check takes the four conditions that read the affinity) */
enum { SC_SINGLE_BY_FALLBACK = 5 };
typedef struct sc_multi_stage {
  int32_t max_spectral_size;         /* 0 = None */
  int32_t spectral_min_embeddings;
  int32_t fallback_type;             /* FallbackClustererType: 1 Agglomerative, 2 Naive */
  double  agglomerative_threshold;   /* read by the Agglomerative type */
  double  naive_threshold;           /* read by the Naive type ... */
  double  naive_adaptation_threshold; /* ... a None arrives as naive_threshold */
  int32_t single_condition;          /* 0: no single-cluster test; 1-4: the values of
                                        sc_single_check.condition; 5: FallbackClusterer */
  double  single_threshold;          /* conditions 2-4 */
  int32_t diagonal_offset;           /* condition 1 */
} sc_multi_stage;
/* sizeof(sc_multi_stage) and the byte offsets of its 9 fields, in declaration order (a binding
 * checks its mirror against them) */
int sc_multi_stage_layout(int* bytes, int* field_offsets);
/* sc_predict_batch_reduced[_naive] generalised (one body runs all three): utterance i is of kind
 *   2  rows < spectral_min_embeddings: the labels are the fallback clusterer's (fallback_type);
 *      no single-cluster test runs; single[i] = -1, route SC_BATCH_ROUTE_FALLBACK, a zeroed diag,
 *   1  max_spectral_size > 0 and rows > max_spectral_size: complete-linkage AHC down to
 *      max_spectral_size clusters; the centroids stay on the device and are clustered as an
 *      utterance of max_spectral_size rows, INCLUDING the single-cluster test (on their rows under
 *      condition 5, on their affinity under conditions 1-4); labels[i][r] = label of row r's
 *      cluster -- zeros when the centroids are found single,
 *   0  everything else: the single-cluster test on the utterance, then the spectral path.
 * Stage A runs kinds 1 and 2 in sc_batch_ahc's / sc_batch_naive_cluster's waves.  The handle's
 * stream is then synchronised -- the centroids are written before anything reads them -- and the
 * sub-batch (the rows of kind 0, the centroid descriptors of kind 1) takes one road:
 * single_condition 0, sc_predict_batch_arrays' grouped form; 1-4, sc_predict_batch_single's body;
 * 5, the verdict waves of sc_predict_batch_single_fallback (fallback_type 1) or
 * sc_predict_batch_single_naive (fallback_type 2) and one grouped batch of the survivors.  Routes,
 * diags and single[i] = 1 / 0 keep each road's convention (conditions 1-4: the route the affinity
 * took and a zeroed diag for a single utterance; condition 5: SC_BATCH_ROUTE_FALLBACK).  The
 * centroids live until the last stage has returned.  Stage A and the verdict waves honour
 * sc_set_reduce_wave_bytes; a member of 4096 rows or more, or one that alone exceeds the budget,
 * keeps sc_ahc's own path.  kinds and single may be NULL.
 * SC_ERR_INVALID before the first launch: group < 2; max_spectral_size == 1 or
 * < spectral_min_embeddings; an unknown fallback_type or single_condition; a Naive threshold
 * pair NaiveClusterer rejects; under condition 1 a member of diagonal_offset >= rows - 1 (kind 1:
 * rows = max_spectral_size); an agglomerative member of one row (kind 2, or kind 0 under condition
 * 5).  The per-member messages carry the utterance's index. */
int sc_predict_batch_multi_stage(sc_handle h, const sc_array* xs, int count, const sc_config* cfg,
                                 const sc_multi_stage* stage, int64_t* const* labels,
                                 sc_diag* diags, int group, int32_t* kinds, int32_t* single);

/*
 * Stream pool:up to `capacity` streaming sessions (multi_stage_clusterer.py:128-180) whose
 * caches stay on the device.  A session lives in a slot 0 .. capacity - 1 and holds up to u2
 * rows of d values; its pre-clusterer reduces them to u1 centroids (2 <= u1 < u2).  All device
 * memory is taken by sc_pool_create, as slabs indexed by slot; SC_ERR_OOM when they do not fit
 * in 85 % of the free memory, so a pool never runs out of memory mid-stream.  A pool works on
 * its handle's stream and, like the handle, is used by one thread at a time; destroy it before
 * the handle.
 */
typedef struct sc_pool_s* sc_pool;
enum { SC_POOL_CACHE = 0, SC_POOL_CENTROIDS = 1 };
int sc_pool_create(sc_handle h, int capacity, int d, int u1, int u2, sc_pool* out);
int sc_pool_destroy(sc_pool pool);
/* the session of `slot` starts again with no rows */
int sc_pool_reset(sc_pool pool, int slot);
/* rows of slot (count of cached rows), or a negative sc_status */
int sc_pool_rows(sc_pool pool, int slot);
/* counts[i] consecutive rows of `rows` (any sc_array with d columns) are appended to the cache
 * of slots[i] (distinct slots), each with its unit-norm copy: one transfer, one launch.  Returns
 * when the source may be reused.  SC_ERR_INVALID, before anything moves, when a cache would
 * exceed u2 rows. */
int sc_pool_append(sc_pool pool, const int32_t* slots, const int32_t* counts, int count,
                   const sc_array* rows);
/* Complete-linkage cosine clustering of every listed slot's cache (more than u1 rows each) down
 * to u1 clusters: labels_out[i] receives the rows(slots[i]) labels, numbered as sklearn numbers
 * them (what sc_ahc returns for those rows); the u1 centroids of each slot stay on the device.
 * One distance pass, one chain launch (a workgroup per slot) and one centroid launch for all. */
int sc_pool_precluster(sc_pool pool, const int32_t* slots, int count, int64_t* const* labels_out);
/* device descriptor (u1 x d, float64) of the centroids the last sc_pool_precluster left */
int sc_pool_centroids(sc_pool pool, int slot, sc_array* out);
/* The agglomerative fallback of a stream that is still short (fallback_clusterer.py:108-113):
 * average-linkage cosine clustering of every listed slot's cache, cut at distance_threshold.
 * labels_out[i] receives the rows(slots[i]) labels: what sc_ahc(x, n, d, SC_LINKAGE_AVERAGE,
 * n_clusters = 0, distance_threshold) returns for those rows; a slot of one row gets label 0.
 * One distance pass and one linkage launch for all slots of up to 128 rows (the distance matrix
 * of each in LDS, a wavefront per slot); larger ones share the pre-clusterer's two kernels in the
 * same call.  Computes no centroids and leaves those of sc_pool_precluster as they are.
 * SC_ERR_INVALID, before anything is launched, for a slot without rows, a slot listed twice or a
 * NULL argument. */
int sc_pool_fallback(sc_pool pool, const int32_t* slots, int count, double distance_threshold,
                     int64_t* const* labels_out);
/* device descriptor (rows(slot) x d, float64, row_stride = d rounded up to 16) of the slot's
 * cache itself, the twin of sc_pool_centroids: valid until the slot is next appended to,
 * compressed or reset.  SC_ERR_INVALID for a slot without rows. */
int sc_pool_cache(sc_pool pool, int slot, sc_array* out);
/* what = SC_POOL_CACHE: the rows(slot) x d cache; SC_POOL_CENTROIDS: the u1 x d centroids */
int sc_pool_get(sc_pool pool, int slot, int what, double* out);
/* dynamic compression: the cache of slot becomes its u1 centroids (copied on the device) */
int sc_pool_compress(sc_pool pool, int slot);

/*
 * Fallback decisions of the callers (fallback_clusterer.py, naive_clusterer.py).
 * sc_affinity_stats: out[4] = {affinity.min(), np.diag(affinity, 1).min(), mean,
 *   np.std(affinity)} of the RESIDENT affinity (fallback_clusterer.py:137-153).
 * sc_affinity_gmm_bic: BIC of sklearn-default 1- and 2-component Gaussian mixtures fitted
 *   to the resident affinity's entries j >= i + diagonal_offset (:154-173).
 * sc_naive_cluster: NaiveClusterer.predict (naive_clusterer.py:57-105) continuing from a
 *   state of *n_centroids centroids (row-major, `capacity` rows >= *n_centroids + n).
 */
int sc_affinity_stats(sc_handle h, double* out);
int sc_affinity_gmm_bic(sc_handle h, int diagonal_offset, double* bic1, double* bic2);
int sc_naive_cluster(sc_handle h, const double* x, int n, int d, double threshold,
                     double adaptation_threshold, double* centroids, int32_t* counts,
                     int32_t* n_centroids, int capacity, int64_t* labels);

/* ---- single stages (ndarray in / ndarray out; parity tests and the
 *      per-op Python classes use these) ------------------------------------- */
/* the ingest alone: out receives the (rows, cols) fp64 values the pipeline sees for `x` */
int sc_stage_ingest(sc_handle h, const sc_array* x, double* out);
/* the affinity ingest alone, on destination memory filled with NaNs: out receives the n rows of
 * matrix_ld(n) doubles as sc_set_affinity_array left them (matrix_ld(n): n rounded up to 16, plus
 * 16 where that is a multiple of 512), padding included, *symmetric the flag of the same pass */
int sc_stage_affinity_ingest(sc_handle h, const sc_array* affinity, double* out, int* symmetric);
/* ... of `count` (<= 64) matrices by ONE grouped launch (host sources staged at their own width
 * first): outs[i] receives member i's rows, symmetric[i] its flag */
int sc_stage_affinity_ingest_group(sc_handle h, const sc_array* affinities, int count,
                                   double* const* outs, int* symmetric);
/* utils.compute_affinity_matrix (utils.py:20-41) */
int sc_stage_affinity(sc_handle h, const double* x, int n, int d, double* out);
/* AffinityRefinementOperation.refine (refinement.py:136-245); op = sc_op,
 * options are read from cfg. */
int sc_stage_refine(sc_handle h, int op, const sc_config* cfg, const double* in,
                    int n, double* out);
/* ConstraintOperation.adjust_affinity (constraint.py:106-118, 138-164); the operator
 * and its options are read from cfg.  Any square affinity / constraint matrix. */
int sc_stage_constraint(sc_handle h, const sc_config* cfg, const double* affinity,
                        const double* constraint_matrix, int n, double* out);
/* the same with the constraint matrix of ConstraintMatrix.compute_diagonals
 * (constraint.py:188-201) given as its band of n - 1 values (sc_set_constraint_band) */
int sc_stage_constraint_band(sc_handle h, const sc_config* cfg, const double* affinity,
                             const double* band, int n, double* out);
/* Test entry: ConstraintPropagation (alpha from cfg) of `count` (1 .. 16) SYMMETRIC affinities with
 * banded constraints as ONE grouped chain, through the launchers sc_predict_batch_constrained uses.
 * Member z: affinities[z] (ns[z], ns[z]) row-major, bands[z] its ns[z] - 1 values, outs[z] receives
 * the adjusted affinity.  ns[z] = 0, or bands[z] = NULL with ns[z] > 1, marks an idle member: its
 * outs[z] is not written.  The call allocates device memory shaped like a member arena (row pitch,
 * work matrices), fills every padding element and workspace with quiet NaNs before the inputs are
 * copied in, runs, and frees.  ns[z] <= 8192. */
int sc_stage_constraint_band_group(sc_handle h, const sc_config* cfg, int count, const int32_t* ns,
                                   const double* const* affinities, const double* const* bands,
                                   double* const* outs);
/* sc_stage_constraint with the constraint matrix given as `count` directed entries
 * (sc_set_constraint_pairs) */
int sc_stage_constraint_pairs(sc_handle h, const sc_config* cfg, const double* affinity,
                              const int32_t* rows, const int32_t* cols, const double* vals,
                              int count, int n, double* out);
/* Test entry: sc_stage_constraint_band_group with member z's constraint given as counts[z] <=
 * ns[z] entries (rows[z], cols[z], vals[z]) instead of a band; the entry buffers are NaN-filled
 * before the upload like everything else.  ns[z] = 0 marks an idle member; counts[z] = 0 is a
 * live member with Q = 0 (outs[z] receives the affinity unchanged).  A member's result is, bit
 * for bit, what the last stage of sc_stage_constraint_pairs makes of the same T. */
int sc_stage_constraint_pairs_group(sc_handle h, const sc_config* cfg, int count,
                                    const int32_t* ns, const double* const* affinities,
                                    const int32_t* const* rows, const int32_t* const* cols,
                                    const double* const* vals, const int32_t* counts,
                                    double* const* outs);
/* sc_stage_constraint with the constraint matrix as a described source (sc_set_constraint_array) */
int sc_stage_constraint_array(sc_handle h, const sc_config* cfg, const double* affinity,
                              const sc_array* constraint_matrix, int n, double* out);
/* Test entry: sc_stage_constraint_band_group with member z's constraint given as a dense SYMMETRIC
 * (ns[z], ns[z]) row-major host matrix constraints[z] (SC_ERR_INVALID for one that is not), in a
 * NaN-filled matrix of the arena's row pitch.  ns[z] = 0 or constraints[z] = NULL marks an idle
 * member.  The last stage is the dense one of a constrained batch's chain: T Q^T by the
 * full-output grouped product, T (T Q^T)^T by the symmetric one, the adjustment. */
int sc_stage_constraint_dense_group(sc_handle h, const sc_config* cfg, int count,
                                    const int32_t* ns, const double* const* affinities,
                                    const double* const* constraints, double* const* outs);
/* Test entry: ONE launch of the grouped two-operand fp64 product on host operands.  Member z:
 * outs[z] = As[z] Bs[z]^T (+ addends[z] when epilogue = 2; epilogue = 0: none) for (ns[z], ns[z])
 * row-major matrices, Bs[z] = NULL (or Bs = NULL): B = A; ns[z] = 0: idle, outs[z] not written.
 * Operands and result live in device matrices of the arena's row pitch ld = ns[z] rounded up to 16
 * (+ 16 when that is a multiple of 512), NaN-filled before the operands go in; outs[z] receives
 * all ns[z] x ld elements of the result buffer, padding columns as the launch left them.
 * full = 0: the symmetric form (upper-triangle tiles, mirror tiles written transposed: commuting
 * symmetric operands); full != 0: every tile (ti, tj) from its own operands.  1 <= count <= 16,
 * ns[z] <= 8192. */
int sc_stage_gemm_pair_group(sc_handle h, int count, const int32_t* ns, const double* const* As,
                             const double* const* Bs, const double* const* addends,
                             double* const* outs, int epilogue, int full);
/* rowmax / rowsum of Diffuse(a) = a a^T (refinement.py:232-234) for a SYMMETRIC (n, n) input --
 * what RowWiseNormalize (refinement.py:240-245) and the Laplacian degree (laplacian.py:41) read
 * of it -- by either route: mode 1 the explicit fp64 product, mode 2 the matrix-free search
 * (n <= 65536).  info (6 ints since ABI 7, may be NULL): candidates evaluated exactly, rows over
 * the candidate cap (evaluated in full), largest candidate count of a row, 1 if S was formed after
 * all, tiles of the digit product computed, tiles in its upper triangle. */
int sc_stage_diffuse_rowstats(sc_handle h, const double* a, int n, int mode, double* rowmax,
                              double* rowsum, int32_t* info);
/* Test entries of the symmetric eigensolver's inner kernels (additions of ABI 8; no reference
 * equivalent -- the reference calls LAPACK).
 *
 * sc_stage_block_operator: ONE application of the solver's block operator, through the launchers
 * the solver itself uses, for `count` (1 .. 16) independent problems, so that tests can hold the
 * product kernels to a high-precision product entry by entry.  Problem z: ns[z] rows (0 = an idle
 * member, grouped form only), matrices[z] (n, n) row-major, vs[z] the block V (n, 8) row-major,
 * ws[z] (n, 8) receives W; cvecs / pvecs / vs_scales (each array, or an entry, may be NULL) hold
 * n-vectors c, p, s with NULL standing for c = 1, p = 0, s = c.  route is an OR of
 * SC_BLOCK_ROUTE_*:
 *   0                          W = p .* V + c .* (M (s .* V)), the full-matrix kernel
 *   SC_BLOCK_ROUTE_SYM         the same from the upper triangle of a symmetric M (slab kernel +
 *                              its reduce)
 *   SC_BLOCK_ROUTE_TWO_PRODUCT W = p .* V + c .* (M (M (s .* V))), the matrix-free Diffuse operator
 *   SC_BLOCK_ROUTE_GROUPED     all problems in one grouped launch instead of one launch each
 * The call allocates device memory shaped like the solver's arena (row pitch, slab workspace),
 * fills every padding element and workspace with quiet NaNs before the inputs are copied in --
 * anything outside the matrix that reaches an accumulator shows in W -- runs, and frees. */
enum {
  SC_BLOCK_ROUTE_SYM = 1,
  SC_BLOCK_ROUTE_TWO_PRODUCT = 2,
  SC_BLOCK_ROUTE_GROUPED = 4
};
int sc_stage_block_operator(sc_handle h, int count, const int32_t* ns,
                            const double* const* matrices, const double* const* cvecs,
                            const double* const* pvecs, const double* const* vs_scales,
                            const double* const* vs, double* const* ws, int route);
/* sc_stage_krylov_state: a read-only copy of what the last block Lanczos solve on this handle
 * (sc_stage_sym_eig, sc_eig_ncluster, sc_predict ... at n > 128 on a symmetric operator; not the
 * members of a grouped batch) left on the device, so that tests can check the chain's invariants
 * at rounding level: the orthonormal basis Q[:, 0:m] -> q (n, m) row-major, the projected operator
 * T = Q^T Op Q -> t (m, m), the Gram matrix of the last residual block -> g (8, 8), and the
 * scaling vectors of Op = diag(p) + diag(c) S diag(c) -> c, p (n each).  info (8 ints): [0] m,
 * [1] n, [2] 1 when S was applied as A A (matrix-free Diffuse: S = A A^T is never formed), [3]
 * block steps the device had run beyond m when the solve ended (then g belongs to block m + 8 *
 * info[3]), [4] restart cycles; the rest 0.  q, t, g, c, p may each be NULL (a first call with
 * info alone sizes the buffers).  SC_ERR_INVALID with a message when the last solve on the handle
 * did not end in block Lanczos (n <= 128: dense Jacobi; the dense tridiagonal routes; the general
 * path) or when no solve has run since the handle was given a new problem. */
int sc_stage_krylov_state(sc_handle h, int32_t* info, double* q, double* t, double* g, double* c,
                          double* p);
/* Test entry of the fused refinement front (addition of ABI 9; no reference equivalent): what
 * the stages between the affinity and the eigensolver leave behind, on each of the three drivers
 * that run them.  It runs the product's own front -- the same functions, the same launch
 * sequence, every routing decision as a full call takes it -- stops before the eigensolver and
 * copies out, per member, into outs[z] (any pointer may be NULL):
 *   a0 (n, n)        the affinity the route computed (or was given)
 *   cropval (n)      CropDiagonal's value vector, from the affinity GEMM's epilogue or from
 *                    k_crop_value (not written when the op ran unfused or is not in the sequence)
 *   cut (n)          the cut vector of RowWiseThreshold
 *   a (n, n)         the refined matrix before Diffuse (thresholded and symmetrised)
 *   s (n, n)         Diffuse(a) = a a^T, where the route formed it
 *   rowmax, rowsum   the row statistics the scaling kernel read
 *   c, p, t (n)      the scaling vectors of Op = diag(p) + diag(c) S diag(c)
 *   info             SC_FRONT_INFO_* below
 * route:
 *   SC_FRONT_ROUTE_SINGLE   count = 1.  xs[0] (ns[0], d): sc_set_embeddings + sc_compute_affinity
 *                           + the front of sc_eig_ncluster.  xs == NULL: `affinity` (ns[0], ns[0])
 *                           through sc_set_affinity instead (no epilogue crop value then).
 *   SC_FRONT_ROUTE_GROUPED  count 1 .. 16 embeddings matrices xs[z] (ns[z], d): the grouped front
 *                           of sc_predict_batch_grouped, one call, members in the order given.
 *   SC_FRONT_ROUTE_SWEEP    one problem xs[0] (ns[0], d) and count (2 .. 16) values p_values[z] of
 *                           p_percentile: the front of one round of sc_eig_ncluster_sweep; outs[z]
 *                           belongs to p_values[z] (a0 and cropval are the shared ones).
 *   SC_FRONT_ROUTE_SHORT_SWEEP  the same for a problem of ns[0] <= 128 rows: the front of one
 *                           launch of (matrix, p) pairs of a short level (k_short_sweep_front,
 *                           cut kernel 4), the Diffuse product through the grouped launcher;
 *                           count 2 .. 64.
 *   SC_FRONT_ROUTE_SHORT_WAVE   count 1 .. 64 embeddings matrices xs[z] (ns[z] <= 128, d <= 512):
 *                           the front of one wave of the short route of sc_predict_batch_grouped
 *                           (k_short_wave_front, cut kernel 5: one launch for the wave between the
 *                           grouped GEMMs), members in the order given.  Every array is bit for
 *                           bit the SINGLE route's for that member alone; cropval is written
 *                           where the single call writes it.  A member above 128 rows, d > 512,
 *                           or a sequence other than [CropDiagonal] [GaussianBlur] RowWiseThreshold
 *                           Symmetrize [Diffuse] [RowWiseNormalize]: SC_ERR_UNSUPPORTED.
 * A configuration the route's grouped code does not cover (a group member below n = 256 or a
 * sequence other than ICASSP2018's; a sweep the product would evaluate one by one) returns
 * SC_ERR_UNSUPPORTED: the entry never takes another path quietly. */
enum { SC_FRONT_ROUTE_SINGLE = 0, SC_FRONT_ROUTE_GROUPED = 1, SC_FRONT_ROUTE_SWEEP = 2,
       SC_FRONT_ROUTE_SHORT_SWEEP = 3, SC_FRONT_ROUTE_SHORT_WAVE = 4 };
enum {
  SC_FRONT_INFO_DIFFUSE_PATH = 0,   /* SC_DIFFUSE_PATH_NONE / _EXPLICIT / _FREE */
  SC_FRONT_INFO_SYMMETRIC = 1,
  SC_FRONT_INFO_FOLDED_ROWNORM = 2, /* RowWiseNormalize folded into the scaling vectors */
  SC_FRONT_INFO_FREE_OP = 3,        /* the solver would apply `a` twice */
  SC_FRONT_INFO_DIGITS_FUSED = 4,   /* the threshold pass wrote the 8-bit digits */
  SC_FRONT_INFO_BLUR_KERNEL = 5,    /* 0 generic, 1 tile, 2 streaming; -1 no blur ran */
  SC_FRONT_INFO_BLUR_ROWS = 6,      /* rows per wave of the streaming kernel, else 0 */
  SC_FRONT_INFO_FREE_CANDIDATES = 7,
  SC_FRONT_INFO_FREE_OVERFLOW_ROWS = 8, /* rows whose statistics the solver's first
                                           synchronisation would still correct */
  SC_FRONT_INFO_FREE_FORMS_S = 9,   /* more of them than the exact-row route takes: the solver
                                       would form S after all */
  SC_FRONT_INFO_CROP_SOURCE = 10,   /* 0 no value vector, 1 GEMM epilogue, 2 k_crop_value */
  SC_FRONT_INFO_CUT_KERNEL = 11,    /* 0 none, 1 k_cut_from_partials, 2 k_cut_from_rows,
                                       3 k_row_percentile_cut, 4 k_short_sweep_front,
                                       5 k_short_wave_front */
  SC_FRONT_INFO_WRITTEN = 12,       /* bit i: the i-th pointer of sc_front_out was filled */
  SC_FRONT_INFO_LAUNCHES = 13,      /* SC_FRONT_ROUTE_SHORT_WAVE: kernel launches the route
                                       enqueued for the whole front of the call (ingest apart);
                                       0 on the other routes */
  SC_FRONT_INFO_COUNT = 16
};
typedef struct sc_front_out {
  double* a0;
  double* cropval;
  double* cut;
  double* a;
  double* s;
  double* rowmax;
  double* rowsum;
  double* c;
  double* p;
  double* t;
  int32_t info[SC_FRONT_INFO_COUNT];
} sc_front_out;
int sc_stage_front(sc_handle h, int route, const sc_config* cfg, int count, const int32_t* ns,
                   int d, const double* const* xs, const double* affinity,
                   const double* p_values, sc_front_out* outs);
/* Test entries of the dense symmetric route (additions of ABI 10; no reference equivalent -- the
 * reference calls LAPACK): Householder tridiagonalisation, Sturm-count multisection and the
 * reflector back-transform, each alone and through the launchers the route itself uses, so that
 * tests can tell an error of one from an error of another.  Like sc_stage_block_operator each
 * call allocates device memory shaped like the solver's arena (row pitch, panel, work vectors,
 * the GEMM's split-K scratch), fills all of it -- padding, workspaces, results -- with quiet NaNs
 * before the inputs are copied in, runs, copies out and frees.
 *
 * sc_stage_tridiag: T = Q^T Op Q for Op = diag(p) + diag(c) m diag(c), m (n, n) symmetric, n >= 32.
 *   c, p (n each) may be NULL: c = 1 / p = 0; both NULL: Op = m, the materialising kernel does
 *   not run.  Outputs (each may be NULL): d (n) the diagonal of T, e (n) its off-diagonal with
 *   e[n-1] = 0, tau (n) the reflector scalars (tau[n-1] = 0), reflectors (n, n) the matrix the
 *   reduction leaves: row j holds v_j in columns j+1 .. n-1 (v_j[j+1] = 1), Q = H_0 ... H_{n-2},
 *   H_j = I - tau_j v_j v_j^T; what the rest of it holds is unspecified.
 * sc_stage_tridiag_values: every eigenvalue of the tridiagonal d (n), e (n - 1; NULL at n = 1),
 *   n >= 1, DESCENDING into values_desc (n).
 * sc_stage_td_backtransform: z (n, cols) row-major <- Q z, with reflectors (n, n) and tau (n) as
 *   sc_stage_tridiag writes them (only columns j+1 .. n-1 of row j are read).  The columns go to
 *   the device column-major and come back through the transposition of sc_get_eigenvectors, as
 *   in a solve.  flags: SC_TD_BACKTRANSFORM_GLOBAL runs the kernel that keeps the column in
 *   global memory -- the product's choice above n = 16384 -- whatever n is. */
enum { SC_TD_BACKTRANSFORM_GLOBAL = 1 };
int sc_stage_tridiag(sc_handle h, const double* m, int n, const double* c, const double* p,
                     double* d, double* e, double* tau, double* reflectors);
int sc_stage_tridiag_values(sc_handle h, const double* d, const double* e, int n,
                            double* values_desc);
int sc_stage_td_backtransform(sc_handle h, const double* reflectors, const double* tau, int n,
                              double* z, int cols, int flags);
/* Test entries of the general (non-symmetric) path (additions of ABI 11; no reference equivalent
 * -- the reference calls np.linalg.eig): the device Hessenberg reduction alone, the Rayleigh-Ritz
 * kernels on given data, and what a block Arnoldi solve left in the arena.  The first two own
 * their device memory like the entries above: arena shapes (row pitch, the basis pitch of 136
 * doubles for Q, Op Q and the coefficient vectors, vectors padded to a multiple of 16), quiet
 * NaNs everywhere before the inputs are copied in.
 *
 * sc_stage_hessenberg: m (n, n) row-major, n >= 1, through the step the dense general route runs
 *   between "matrix in scratch" and "packed matrix and tau on the host": the read-back of
 *   max|a|, the power-of-two scaling of a matrix beyond 2^+-400, the reduction.  Outputs (each
 *   may be NULL): packed (n, n) in LAPACK dgehd2 storage (H on and above the subdiagonal,
 *   v_k[k+2 ..] below it in column k, v_k[k+1] = 1 implied), tau (n), scale (1 double): the
 *   factor the eigenvalues of H get back, 1.0 when nothing was scaled.
 * sc_stage_general_ritz: q, opq (n, m) row-major, yre, yim (m, cols), theta_re, theta_im (cols),
 *   1 <= cols <= m <= 128.  q = NULL is the identity form of the dense solver (m = n <= 64).
 *   Outputs (each may be NULL): vre, vim (n, cols) = Q Y after k_gen_ritz; resid (cols) =
 *   ||Op Q y - theta Q y||_2, 32 pairs per launch as the solver runs them (needs q, opq, theta);
 *   pre, pim (n, cols) the vectors after k_gen_phase and e (n, cols) the real-part copy it
 *   writes.  codes (8 ints: -1 noise, else 2 * column + part, part 1 = imaginary) with w (n, 8):
 *   the restart block k_gen_gather builds from the phased vectors with `seed`; both or neither.
 * sc_stage_arnoldi_state: read-only, like sc_stage_krylov_state.  After a solve that ended in
 *   SC_EIG_PATH_BLOCK_ARNOLDI: info (8 ints) = [0] m, [1] n, [2] 1 for the wide form, [3] restart
 *   cycles, [4] block passes, [5] 1 when the operator had its sign turned; q, opq (n, m)
 *   row-major, hm (m, m) the projected matrix of the final check, cl, cr, p (n each) the scalings
 *   of Op x = p .* x + cl .* (M (cr .* x)) as the solve used them.  Any of them but info may be
 *   NULL.  SC_ERR_INVALID after any other kind of solve. */
int sc_stage_hessenberg(sc_handle h, const double* m, int n, double* packed, double* tau,
                        double* scale);
int sc_stage_general_ritz(sc_handle h, const double* q, const double* opq, int n, int m,
                          const double* yre, const double* yim, const double* theta_re,
                          const double* theta_im, int cols, double* vre, double* vim,
                          double* resid, double* pre, double* pim, double* e,
                          const int32_t* codes, uint64_t seed, double* w);
int sc_stage_arnoldi_state(sc_handle h, int32_t* info, double* q, double* opq, double* hm,
                           double* cl, double* cr, double* p);
/* laplacian.compute_laplacian (laplacian.py:24-60) */
int sc_stage_laplacian(sc_handle h, int laplacian_type, const double* in, int n,
                       double* out);
/*
 * utils.compute_sorted_eigenvectors (utils.py:44-71) for a SYMMETRIC input:
 * the `count` largest (descend=1) or smallest (descend=0) eigenpairs.
 * values: count doubles; vectors: (n, count), unit 2-norm columns, or NULL for values
 * only -- then count may be anything up to n (count > 64 at n > 128 takes the dense
 * tridiagonalisation path: what np.linalg.eigvalsh returns).
 */
int sc_stage_sym_eig(sc_handle h, const double* m, int n, int count, int descend,
                     double* values, double* vectors, sc_diag* diag);
/*
 * utils.compute_sorted_eigenvectors (utils.py:44-71) for ANY square input: what
 * np.linalg.eig + .real + argsort give -- real parts of the `count` eigenvalues of
 * largest (descend=1) / smallest (descend=0) real part and the real parts of their
 * eigenvectors, normalised like LAPACK dgeev (unit 2-norm, largest component of a
 * complex vector real).  n <= 64: Hessenberg + complex QR in one wavefront (all pairs
 * available); larger n: block Arnoldi, count <= 32.
 */
int sc_stage_eig(sc_handle h, const double* m, int n, int count, int descend,
                 double* values, double* vectors, sc_diag* diag);
/*
 * The building blocks on described arrays: each is the ingest of its input (sc_set_embeddings_array's
 * / sc_set_affinity_array's sources and errors), the launches of the double* entry above, and the
 * egress of the result into `out` -- an sc_array in host or device memory, fp64 / fp32 / fp16 /
 * bf16, of exactly the result's shape, with non-negative element strides that map no two indices
 * to one address: over the dimensions of more than one element, ordered by stride, the small
 * stride is >= 1 and the big one >= small stride x extent of the small one (SC_ERR_INVALID
 * otherwise, before anything is launched).  Narrowing is fp64 -> fp32 round to nearest even, then
 * fp32 -> fp16 / bf16 round to nearest even (PyTorch's tensor.to(dtype)): overflow to +-inf, signed
 * zeros and subnormals of every width kept, NaN stays NaN.  The results are, bit for bit, the
 * double* entry's on the widened values, narrowed.  Only elements of the view are written.  The
 * input is completely inside the handle's buffers before the first byte of `out` is written: `out`
 * may be the input, any view of it, or overlap it.  All return with the stream drained.
 */
/* utils.compute_affinity_matrix: x (n, d) -> out (n, n) */
int sc_stage_affinity_array(sc_handle h, const sc_array* x, const sc_array* out);
/* AffinityRefinementOperation.refine: in (n, n) -> out (n, n); op and cfg as sc_stage_refine */
int sc_stage_refine_array(sc_handle h, int op, const sc_config* cfg, const sc_array* in,
                          const sc_array* out);
/* laplacian.compute_laplacian: in (n, n) -> out (n, n) */
int sc_stage_laplacian_array(sc_handle h, int laplacian_type, const sc_array* in,
                             const sc_array* out);
/* utils.compute_sorted_eigenvectors: in (n, n) -> values (1, count), vectors (n, count).  The
 * symmetric / general decision -- np.allclose(m, m.T, rtol=0, atol=1e-12 * max(max|m|, 1e-300)) on
 * the widened fp64 values, a matrix with a NaN is not symmetric -- is made on the device from one
 * pass that leaves max|m|, max|m_ij - m_ji| and a flag; sc_stage_sym_eig or sc_stage_eig runs
 * accordingly, *symmetric (may be NULL) says which.  count = -1 asks for the default count, which
 * follows the decision (symmetric: n up to 128, else 64; general: n up to 64, else 32): values and
 * vectors then have the symmetric default's columns, the leading columns of the count taken are
 * written, and *symmetric (required) tells the caller which it was -- one pass over the input.
 * count = 0 (values and vectors are not read, *symmetric required) makes the decision alone. */
int sc_stage_eig_array(sc_handle h, const sc_array* in, int count, int descend,
                       const sc_array* values, const sc_array* vectors, int* symmetric);
/* the egress alone (a test entry, the twin of sc_stage_ingest): host_src, (rows, cols) doubles in
 * rows, is uploaded into a buffer at the library's own pitch filled with NaNs first -- rows of
 * matrix_ld(cols) doubles, or with column_major the eigenvector layout E[c * round_up(rows, 16) + r]
 * -- and leaves through the egress into `out` (rows, cols). */
int sc_stage_egress(sc_handle h, const double* host_src, int rows, int cols, int column_major,
                    const sc_array* out);
/*
 * Labels and centroids where the caller wants them.
 *
 * A LABEL ARRAY is an sc_array of one row: rows = 1, cols = n, col_stride >= 0 the step between
 * entries in elements (row_stride addresses nothing), in host memory or on the handle's device.
 * As an input its dtype is SC_DTYPE_I64 or SC_DTYPE_I32, or SC_DTYPE_F64 / SC_DTYPE_F32 holding
 * integral values (predict() returns float64 labels for a size-reduced utterance); as an output
 * SC_DTYPE_I64 or SC_DTYPE_I32 with col_stride >= 1 (n > 1).
 *
 * sc_cluster_centroids_arrays: utils.get_cluster_centroids (reference utils.py:159-176) for
 * `count` >= 1 members in one call.  Member i has embeddings xs[i] (whatever
 * sc_set_embeddings_array takes; all members the same d; a device source is read in place, host
 * sources of the call travel in one copy at their own width), labels labels[i] of xs[i].rows
 * entries, and the result outs[i]: fp64 / fp32 / fp16 / bf16, host or device, outs[i].cols = d,
 * outs[i].rows >= k_i = max(labels[i]) + 1, strides under sc_stage_*_array's rule.  Rows 0 .. k_i - 1
 * of outs[i] are written and nothing else; ks[i] (ks may be NULL) returns k_i.  With outs = NULL
 * (ks required) the call validates the labels and returns the k_i alone, for a caller that has to
 * allocate first.
 *   out[c][f] is the sum from 0.0 of the widened fp64 values x[r][f] over the rows r with
 *   label c, in ascending r, divided by their number -- the bits of np.mean(x[labels == c],
 *   axis=0) and of sc_cluster_centroids -- narrowed by sc_stage_*_array's rule.  A label in
 *   0 .. k - 1 that no row carries gives a row of NaN (0 / 0, as the reference); rows with a
 *   negative label belong to no cluster (the reference's `labels == c` never matches them).
 * Two steps: one pass over all members' labels (validation, k_i; device labels by one kernel, host
 * labels on the host), then a stable counting sort of each member's labels on the device and the
 * means from each cluster's own rows.  At most three launches per 32768 members and two
 * synchronisations of the stream, whatever `count` is.  SC_ERR_INVALID with a message that names
 * the member's index, before a byte of any outs[i] is written: a label array that does not hold
 * xs[i].rows entries; a float label that is not integral or not finite; a label of 2^31 - 1 or
 * more; outs[i].cols != d; outs[i].rows < k_i; an outs[i] in device memory whose byte range
 * overlaps a device xs[j] or labels[j] of the call.  Returns with the stream drained.
 */
int sc_cluster_centroids_arrays(sc_handle h, const sc_array* xs, const sc_array* labels, int count,
                                const sc_array* outs, int32_t* ks);
/* Labels out: labels[i] (int64, host, outs[i].cols entries -- what every predict entry returns)
 * into the label array outs[i], for `count` >= 1 members.  Host destinations are written on the
 * host; the device destinations of the call take one upload, one launch per 32768 of them and one
 * synchronisation.  Every descriptor is checked before anything is written; only the entries of
 * the views are written.  An int32 destination takes the low 32 bits (labels are cluster numbers
 * below n). */
int sc_labels_egress(sc_handle h, const int64_t* const* labels, int count, const sc_array* outs);
/* numpy.random.RandomState(seed).random_sample(count): the MT19937 stream that
 * sklearn's KMeans(random_state=0) (custom_distance_kmeans.py:39-43) consumes.
 * Host-only; exported so the stream can be pinned without a GPU. */
int sc_random_state_doubles(uint32_t seed, int count, double* out);
/* index RandomState.choice(n, p=uniform) returns for the uniform draw u:
 * cumsum(1/n) / cdf[-1], searchsorted(u, side="right") (first k-means++ centre) */
int sc_uniform_choice(int n, double u);
/* The host routine that solves the small (<= 64 x 64) Rayleigh-Ritz problems of the block
 * Lanczos solver: symmetric a (m x m, row-major) -> eigenvalues ascending, eigenvectors in
 * the columns of `vectors` (Householder tridiagonalisation + implicit QL).  Host-only;
 * exported so it can be pinned without a GPU. */
int sc_host_symmetric_eig(const double* a, int m, double* values, double* vectors);
/* The Rayleigh-Ritz solve of larger bases (64 < m <= 128): ALL eigenvalues of the symmetric
 * m x m matrix `a` (row-major; upper triangle read), descending, and the eigenvectors of the
 * leading `need` of them ((m, need) row-major): Householder tridiagonalisation with kept
 * reflectors + QL for the values + inverse iteration + back-transform.  Host-only. */
int sc_host_symmetric_eig_partial(const double* a, int m, int need, double* values,
                                  double* vectors);
/* Eigenvectors of the symmetric tridiagonal matrix (d[0..n), e[0..n-1)) for the k given
 * eigenvalues `lam` by inverse iteration (LAPACK dstein's method): vectors is (n, k)
 * row-major, column q belongs to lam[q], unit 2-norm.  The host step of the dense landing
 * pad (SC_EIG_PATH_DENSE_FULL) that takes over whenever block Lanczos gives up, so that
 * predict() returns wherever np.linalg.eig (utils.py:59) does.  Host-only; exported so it
 * can be pinned without a GPU. */
int sc_host_tridiag_eigvectors(const double* d, const double* e, int n, const double* lam,
                               int k, double* vectors);
/* The Rayleigh-Ritz solve of the WIDE block Arnoldi (general eigen path, more than 32 eigenpairs
 * at n > 64: projected problems of order 64 < m <= 128; smaller ones are solved by a
 * one-wavefront device kernel): eigenvalues of the real m x m matrix `a` (row-major) sorted by
 * real part, descending, and the first nvec eigenvectors ((m, nvec) row-major, real and
 * imaginary parts, unit 2-norm).  Hessenberg reduction + shifted complex QR + back
 * substitution.  Host-only; exported so it can be pinned against numpy without a GPU. */
int sc_host_general_eig(const double* a, int m, int nvec, double* values_re, double* values_im,
                        double* vectors_re, double* vectors_im);
/* The same contract in real arithmetic -- Householder Hessenberg reduction, double-shift QR for
 * the values, inverse iteration + back-transform for the nvec leading vectors: what the
 * Rayleigh-Ritz checks of block Arnoldi (every basis size, general eigen path; replaces
 * np.linalg.eig of utils.py:59 on the projected problem) call since round 6; the function above is
 * its fallback when an inverse iteration does not converge.  Host-only; exported so it can be
 * pinned against numpy without a GPU. */
int sc_host_general_eig_fast(const double* a, int m, int nvec, double* values_re,
                             double* values_im, double* vectors_re, double* vectors_im);
/* The host half of the dense general eigensolver for n > 64 (SC_EIG_PATH_DENSE_HESSENBERG;
 * replaces np.linalg.eig, utils.py:59, where more eigenvalues of a non-symmetric matrix are read
 * than a Krylov basis holds).  `packed` (n, n) row-major: an upper Hessenberg matrix on and
 * above the subdiagonal and, below it, the Householder reflectors that produced it (LAPACK
 * dgehd2's storage, what the device reduction leaves), tau (n - 2).  values: all n eigenvalues
 * (implicit double-shift QR, unordered); vectors_re / vectors_im ((n, count) row-major): the
 * eigenvectors of the ORIGINAL matrix for the eigenvalues values[pick[q]] -- inverse iteration on
 * the Hessenberg form + back-transform through the reflectors, not normalised; *max_resid: the
 * largest relative residual on the Hessenberg form.  Host-only; exported so it can be pinned
 * against numpy without a GPU. */
int sc_host_hessenberg_eig(const double* packed, const double* tau, int n, int count,
                           const int32_t* pick, double* values_re, double* values_im,
                           double* vectors_re, double* vectors_im, double* max_resid);
/* The eigensolver's stopping rule for one Ritz value (eig_driver.hip): a bound on the distance
 * from theta[i] (Ritz values of a SYMMETRIC operator, descending) to the eigenvalue it
 * approximates, from the residual norms resid[] -- resid[i] itself, or the Kato-Temple bound
 * resid[i]^2 / delta where the neighbouring Ritz values fence theta[i] off.  Host-only;
 * exported so the bound can be checked against true Rayleigh-Ritz errors without a GPU.
 * Returns the bound through *bound. */
int sc_host_value_error_bound(const double* theta, const double* resid, int m, int i,
                              double* bound);
/* AutoTune's search state (autotune.py:29-38): the p_percentile range, the step of its grid, the
 * number of search levels and the proxy that is minimised. */
#define SC_AUTOTUNE_PERCENTILE_OVER_NME 1      /* (1 - p) / g, g the largest eigengap */
#define SC_AUTOTUNE_PERCENTILE_SQRT_OVER_NME 2 /* sqrt(1 - p) / g */
typedef struct sc_autotune {
  double p_min, p_max, step;
  int32_t levels, proxy;
} sc_autotune;
/* One level's values, evaluated by the caller: ratios_out[i] = the proxy at ps[i].  Returns
 * SC_OK, or a status that ends the search and is returned from it. */
typedef int (*sc_autotune_evaluate)(const double* ps, int count, double* ratios_out, void* user);
/* AutoTune.ratio (spectral_clusterer.py:281-286): the proxy of one evaluation whose largest
 * eigengap is max_delta.  Host-only. */
int sc_host_autotune_ratio(const sc_autotune* at, double p, double max_delta, double* ratio);
/* AutoTune.tune (autotune.py:76-132) from the state *at: the grid of a level is
 * np.linspace(p_min, p_max, ceil((p_max - p_min) / step)) to the last bit, values already
 * searched (exact double equality) are not evaluated again, the first strict minimum of a level
 * wins, and unless the grid is empty, holds one value or step < 1e-4 the range narrows to
 * max(2, len / 8) grid points either side of the winner with half the step.  *best_p /
 * *best_index: the winner and its index in its level's grid; *last_p: the last value evaluated;
 * *narrowed: the state tune() leaves in the AutoTune object (*at itself is not written).  Any of
 * the four may be NULL.  SC_ERR_INVALID where tune() raises (no level, no finite ratio, a
 * non-finite grid size).  Host-only; exported so the search can be pinned against
 * AutoTune.tune without a GPU. */
int sc_host_autotune_search(const sc_autotune* at, sc_autotune_evaluate evaluate_many, void* user,
                            double* best_p, int* best_index, double* last_p,
                            sc_autotune* narrowed);
/* A batch in which every utterance is an AutoTune search (a Python loop of predict(u, c) on a fresh
 * clusterer per utterance): every utterance is searched from the state *at, which is not written.
 * bands: NULL, or per utterance the band of its ConstraintMatrix (n_i - 1 values; NULL: none), used
 * when cfg names a constraint.  best_p / last_p (either may be NULL): per utterance the winning
 * p_percentile and the last value its search evaluated.  Routes (sc_last_batch_routes):
 *   2  n <= 128, the two sequences sc_eig_ncluster_sweep groups: waves of up to 64 utterances,
 *      level by level -- fronts per utterance on the member streams (the band applied per
 *      utterance), then ALL (utterance, p) pairs of the wave's current level in launches of up
 *      to 64 (one front launch, one Jacobi launch, a workgroup per pair),
 *      sc_host_autotune_search per utterance on the ratios; the winners' eigenvectors from one
 *      more launch, then the lockstep k-means
 *   1  128 < n < 4096: dealt longest-first to three lanes, each a handle, stream and host thread of
 *      its own running per utterance what predict() runs (ingest, sc_apply_constraint, the levels
 *      through sc_eig_ncluster_sweep, sc_sweep_adopt or one evaluation, sc_cluster)
 *   0  n >= 4096, other sequences, members that left their route: the same per-utterance function
 *      on h; and everything when hipMemGetInfo says the arenas do not fit
 * Every descriptor is validated before the first launch; no constraint is resident in h or in any
 * arena when the call returns, whatever it returns.  group: >= 2 (the grouped form). */
int sc_predict_batch_autotune(sc_handle h, const sc_array* xs, const double* const* bands,
                              int count, const sc_config* cfg, const sc_autotune* at,
                              int64_t* const* labels, sc_diag* diags, double* best_p, int group,
                              double* last_p);
/* utils.compute_number_of_clusters (utils.py:74-130) -- host scalar loop */
int sc_eigengap(const double* eigenvalues, int count, int max_clusters,
                double stop_eigenvalue, int eigengap_type, int descend,
                int* n_clusters, double* max_delta);
/* custom_distance_kmeans.run_kmeans (custom_distance_kmeans.py:13-52),
 * custom_dist="cosine": sklearn k-means++ (RandomState(0)) + one Lloyd step
 * for the seeds, then the cosine loop.  e: (n, k).  centroids_out may be
 * NULL, else (k, k) final centroids. */
int sc_stage_kmeans(sc_handle h, const double* e, int n, int k, int max_iter,
                    int64_t* labels, double* centroids_out, int* iterations);
/* the same with custom_dist = SC_KMEANS_* */
int sc_stage_kmeans_metric(sc_handle h, const double* e, int n, int k, int max_iter,
                           int metric, int64_t* labels, double* centroids_out,
                           int* iterations);
/* sc_stage_kmeans (cosine) with what its kernels compute on the way, for tests.  form: which
 * kernels run -- SC_KMEANS_FORM_AUTO as sc_stage_kmeans chooses, _CHAIN the chain of short
 * kernels (SC_ERR_UNSUPPORTED when it does not take this (n, k): k > 32 or too many rows),
 * _SINGLE the single-workgroup kernel (its large-k form above 64 clusters); the argument
 * decides, not the process-wide switch.  *form_run: 1 chain, 2 single-workgroup, 3 its large-k
 * form.  Every output but labels may be NULL.  All forms: seeds [k] (the k-means++ rows),
 * *iterations, centroids [k * k], labels [n].  The chain alone (left untouched otherwise):
 * col_means [k]; last_candidates / last_potentials [8]: the candidate rows of the last k-means++
 * round and their potentials (the first 2 + int(log k) of each; k = 1: none);
 * lloyd_centroids [k * k] after the sklearn Lloyd step; first_labels [n], the assignment of
 * pass 0; mean_dist[p], p < min(*iterations, mean_dist_cap), the mean distance of pass p.  The
 * chain is enqueued as pass 0, passes 1-3, then four passes at a time. */
#define SC_KMEANS_FORM_AUTO 0
#define SC_KMEANS_FORM_CHAIN 1
#define SC_KMEANS_FORM_SINGLE 2
int sc_stage_kmeans_trace(sc_handle h, const double* e, int n, int k, int max_iter, int form,
                          int* form_run, double* col_means, int* seeds, int* last_candidates,
                          double* last_potentials, double* lloyd_centroids,
                          int64_t* first_labels, double* mean_dist, int mean_dist_cap,
                          int* iterations, double* centroids, int64_t* labels);
/* sc_stage_kmeans_trace with custom_dist = SC_KMEANS_* (sc_stage_kmeans_trace is this call with
 * SC_KMEANS_COSINE): _CHAIN runs the chain with the metric's distance in its assignment (what a
 * grouped batch under sc_set_batch_any_metric runs), _SINGLE the single-workgroup kernel with it
 * (what sc_stage_kmeans_metric runs for a metric other than cosine), _AUTO what
 * sc_stage_kmeans_metric chooses.  Outputs as there. */
int sc_stage_kmeans_trace_metric(sc_handle h, const double* e, int n, int k, int max_iter,
                                 int form, int metric, int* form_run, double* col_means,
                                 int* seeds, int* last_candidates, double* last_potentials,
                                 double* lloyd_centroids, int64_t* first_labels,
                                 double* mean_dist, int mean_dist_cap, int* iterations,
                                 double* centroids, int64_t* labels);
/* The grouped chain (one launch per phase for up to 16 independent problems, as the grouped
 * batch runs it) with the same outputs per member.  es: the members' (ns[z], ks[z]) row-major
 * inputs one after the other; ns[z] = 0 is an idle position.  Outputs are packed by position z:
 * col_means and seeds at z * 32, last_candidates and last_potentials at z * 8, lloyd_centroids
 * and centroids at z * 1024, mean_dist at z * mean_dist_cap, iterations at z; first_labels and
 * labels hold the members' rows one after the other.  A member that met its stop rule goes idle
 * for the later enqueues.  SC_ERR_UNSUPPORTED when the chain does not take a member. */
int sc_stage_kmeans_trace_group(sc_handle h, const double* es, const int* ns, const int* ks,
                                int count, int max_iter, double* col_means, int* seeds,
                                int* last_candidates, double* last_potentials,
                                double* lloyd_centroids, int64_t* first_labels,
                                double* mean_dist, int mean_dist_cap, int* iterations,
                                double* centroids, int64_t* labels);
/* ... with custom_dist = SC_KMEANS_*, one metric for all members (a batch has one sc_config);
 * outputs and packing as sc_stage_kmeans_trace_group, which is this call with SC_KMEANS_COSINE */
int sc_stage_kmeans_trace_group_metric(sc_handle h, const double* es, const int* ns,
                                       const int* ks, int count, int max_iter, int metric,
                                       double* col_means, int* seeds, int* last_candidates,
                                       double* last_potentials, double* lloyd_centroids,
                                       int64_t* first_labels, double* mean_dist,
                                       int mean_dist_cap, int* iterations, double* centroids,
                                       int64_t* labels);
/* custom_distance_kmeans.run_kmeans (:13-52) / CustomKMeans.predict (:85-141) on an (n, dim)
 * input, dim independent of k.  init_centroids (k, dim) row-major, or NULL = sklearn k-means++
 * seeds + one Lloyd step.  centroids_out (k, dim) may be NULL: the centroids of the last
 * assignment pass (what the reference leaves in self.centroids).  *iterations = distance
 * passes run (1 = stopped by the rule after the first pass), as sc_stage_kmeans reports. */
int sc_stage_kmeans_general(sc_handle h, const double* x, int n, int dim, int k, int max_iter,
                            int metric, double tol, const double* init_centroids,
                            int64_t* labels, double* centroids_out, int* iterations);
/* sc_stage_kmeans_general on a described source: x is (n, dim) in host or device memory, fp64 /
 * fp32 / fp16 / bf16, any non-negative element strides.  It is widened exactly on the device
 * into the kernels' column-major layout (a device source is read in place on the handle's
 * stream, a host source is copied at its own width first), so the results are bit for bit those
 * of the same values passed as double*.  Compact host fp64 rows take sc_stage_kmeans_general's
 * own copy.  init_centroids and the outputs are host fp64 as there.  SC_ERR_INVALID before any
 * copy or launch for: an unknown dtype or location, a negative stride, NULL data, a device
 * pointer that is not memory of the handle's device, rows * cols > 2^31 - 1.  The source is not
 * modified and may be reused when the call returns. */
int sc_stage_kmeans_general_array(sc_handle h, const sc_array* x, int k, int max_iter, int metric,
                                  double tol, const double* init_centroids, int64_t* labels,
                                  double* centroids_out, int* iterations);
/* sc_stage_kmeans_metric on a described source: e is the (n, k) spectral embedding, k = e->cols;
 * sources, checks and results as sc_stage_kmeans_general_array. */
int sc_stage_kmeans_metric_array(sc_handle h, const sc_array* e, int max_iter, int metric,
                                 int64_t* labels, double* centroids_out, int* iterations);
/* the k-means ingest alone (a test entry, the twin of sc_stage_ingest): out receives the
 * round_up(rows, 16) x cols doubles the k-means kernels are handed for x, column-major
 * (out[j * ld + r], ld = round_up(rows, 16)), written over memory filled with NaNs: rows
 * 0 .. rows - 1 of every column are the widened values, the rest of the column is zero.
 * (Compact host fp64 rows go through the same kernels here; the k-means entries keep their
 * copy + transposition for them, which leaves the rest of a column unwritten.) */
int sc_stage_ingest_columns(sc_handle h, const sc_array* x, double* out);
/* Every form of the nearest-neighbour-chain linkage (sc_ahc, sc_batch_ahc, the stream pool,
 * sc_batch_fallback_check) on the caller's COSINE matrices, for tests: each form runs its own
 * 1 - clip(c) step and its linkage kernel through the launches production uses, on a descriptor
 * table / pool slabs laid out by hand.  form:
 *   _SINGLE         sc_ahc's distance kernel + chain kernel, one member after the other
 *   _BATCH          sc_batch_ahc's distance kernel + chain kernel (a workgroup per member)
 *   _BATCH_LDS      sc_batch_ahc's LDS kernel (a wavefront per member)
 *   _POOL           the stream pool's distance kernel + chain kernel (position i of the launch
 *                   works in slot count - 1 - i)
 *   _POOL_LDS       the stream pool's LDS kernel
 *   _CHAIN_VERDICT  sc_batch_fallback_check's distance kernel + chain kernel in its verdict form
 *   _LDS_VERDICT    ... its LDS kernel in its verdict form
 * method: SC_LINKAGE_*; the LDS forms take members of at most 128 rows, they and the verdict forms
 * average linkage only.  ns [count]: rows of each member (a member of fewer than 2 rows is left
 * alone); cosines: the members' (n_i, n_i) row-major matrices one after the other.  On the device
 * every matrix has a pitch above n_i, and its padding columns and rows hold what a scan would take
 * for the smallest distance -- cosine 1 (distance 0) for the LDS forms, which turn cosines into
 * distances while they load them, and -1 for the others, whose distance kernel works on the
 * n_i x n_i part alone and whose chain kernel would read the padding as it is: a kernel that
 * looked beyond column n_i would pick one.  first: the table offset of the batch and LDS
 * launches -- members before it are not worked on (forms _SINGLE and _POOL: 0).  bad (may be NULL; not for
 * the pool forms): the members' `bad` words, nonzero = left alone.  threshold: of the verdict
 * forms.  Outputs hold what the caller put there wherever a member was left alone.  Z (forms
 * without a verdict): the members' raw merge lists one after the other, max(n_i - 1, 0) rows of
 * (slot x < slot y, height, size) in chain order.  records (verdict forms): {height, verdict} per
 * member.  labels (may be NULL; forms without a verdict): n_i labels per member, ahc_tree_cut of
 * its Z for n_clusters > 0 or, n_clusters == 0, distance_threshold -- sc_ahc's host half.
 * SC_ERR_HIP when a kernel wrote behind a member's cluster sizes or behind its chain (where
 * sc_ahc keeps the `bad` word).  Every argument is checked before the first launch. */
#define SC_LINKAGE_FORM_SINGLE 0
#define SC_LINKAGE_FORM_BATCH 1
#define SC_LINKAGE_FORM_BATCH_LDS 2
#define SC_LINKAGE_FORM_POOL 3
#define SC_LINKAGE_FORM_POOL_LDS 4
#define SC_LINKAGE_FORM_CHAIN_VERDICT 5
#define SC_LINKAGE_FORM_LDS_VERDICT 6
int sc_stage_linkage(sc_handle h, int form, int method, int count, const int32_t* ns,
                     const double* cosines, int first, double threshold, const int32_t* bad,
                     double* Z, double* records, int64_t* labels, int n_clusters,
                     double distance_threshold);
/* The (n, n) cosine distances sc_ahc (route 0: row normalisation, the symmetric single-call
 * product, 1 - clip) and sc_batch_ahc (route 1: the batched normalisation, the grouped product,
 * the batched 1 - clip, on a wave of this one member) hand to their linkage kernels, for tests.
 * x: (n, d), n >= 2. */
int sc_stage_cosine_distances(sc_handle h, int route, const double* x, int n, int d, double* out);

/* ---- multi-GPU: replicas of the path over the GPUs of one node ------------------------
 * The reference has no distributed layer (a batch is a Python `for` over predict(),
 * SURVEY.md 3.4; AutoTune evaluates its p grid serially, autotune.py:98-111).  Independent
 * units are partitioned over GPUs by the host (spectralcluster_amd/multigpu.py); these
 * entry points are the only communication it needs, on RCCL over xGMI.  Host buffers in
 * and out (staged through the device on the handle's stream); every call returns after
 * its result is on the host.  librccl is opened on first use. */
#define SC_COMM_ID_BYTES 128
typedef struct sc_comm_s* sc_comm;
/* 1 when librccl could be opened */
int sc_comm_available(void);
/* rank 0: ncclGetUniqueId; the 128 bytes reach the other ranks out of band (file/socket) */
int sc_comm_unique_id(unsigned char* id);
/* one process per GPU: join a communicator of world_size ranks on the handle's device;
 * collectives run on the handle's stream */
int sc_comm_init_rank(sc_handle h, int world_size, int rank, const unsigned char* id,
                      sc_comm* out);
/* one process driving ndev GPUs (ncclCommInitAll): out[i] is bound to handles[i] */
int sc_comm_init_all(sc_handle* handles, int ndev, sc_comm* out);
int sc_comm_destroy(sc_comm c);
int sc_comm_rank(sc_comm c);
int sc_comm_size(sc_comm c);
const char* sc_comm_last_error(sc_comm c);
/* root's `bytes` bytes of buf reach every rank's buf (embeddings, packed sc_config) */
int sc_comm_broadcast(sc_comm c, void* buf, size_t bytes, int root);
/* recv (world_size * bytes) = every rank's send (bytes), in rank order (label slabs,
 * AutoTune (ratio, n_clusters) pairs) */
int sc_comm_allgather(sc_comm c, const void* send, void* recv, size_t bytes);
/* element-wise max over ranks, in place (the bench's max-over-ranks time) */
int sc_comm_allreduce_max(sc_comm c, double* values, int count);
/* every rank's stream has drained and every rank has arrived */
int sc_comm_barrier(sc_comm c);

#ifdef __cplusplus
}
#endif
#endif /* SPECTRALCLUSTER_AMD_H_ */
