"""predict() from an affinity instead of embeddings, composed from the oracle's own stages
(`spectral_oracle.predict` with its first line -- `a = affinity(x)` -- taken out): what
`SpectralClusterer.predict_affinity` has to reproduce."""

import typing

import numpy as np

import spectral_oracle as so


def predict_from_affinity(a: np.ndarray, cfg: so.OracleConfig,
                          constraint_matrix: typing.Optional[np.ndarray] = None,
                          autotune: typing.Optional[tuple] = None,
                          dump: typing.Optional[dict] = None) -> np.ndarray:
  """Labels of the reference pipeline fed the (n, n) affinity `a` (widened to float64).
  `autotune` = (p_min, p_max, step, search_level, sqrt_proxy) as in `so.predict`.  `dump`
  receives what `so.eig_ncluster` dumps (eigenvalues among it), n_clusters and best_p."""
  a = np.array(a, dtype=np.float64)
  if a.ndim != 2 or a.shape[0] != a.shape[1]:
    raise ValueError("affinity must be a square matrix")
  if (cfg.constraint_name != so.CONSTRAINT_NONE and cfg.apply_before_refinement
      and constraint_matrix is not None):
    a = so.adjust_affinity(a, constraint_matrix, cfg)
  if autotune is not None:
    v, k, best_p, _ = so.autotune_search(a, cfg, *autotune, constraint_matrix=constraint_matrix)
    if dump is not None:
      dump["best_p"] = best_p
  else:
    v, k, _ = so.eig_ncluster(a, cfg, dump, constraint_matrix)
  if cfg.min_clusters is not None:
    k = max(k, cfg.min_clusters)
  emb = v[:, :k]
  if cfg.row_wise_renorm:
    emb = emb / np.linalg.norm(emb, axis=1, ord=2)[:, None]
  if dump is not None:
    dump["n_clusters"] = k
  return so.run_kmeans(emb, k, cfg.max_iter)


def eigengap_margin(w: np.ndarray, cfg: so.OracleConfig, descend: bool) -> float:
  """How far the eigengap decision on eigenvalues `w` is from a tie: (largest gap - second
  largest) / largest, over the gaps the rule compares.  Inputs whose labels a test pins should
  have a margin far above the solver's tolerance."""
  w = np.asarray(w, dtype=np.float64)
  end = len(w)
  if cfg.max_clusters and cfg.max_clusters + 1 < end:
    end = cfg.max_clusters + 1
  ratio = cfg.eigengap_type == so.EIGENGAP_RATIO
  wmax = np.max(w)
  gaps = []  # so.eigengap's candidates, in its order
  if descend:
    for i in range(1, end):
      if w[i - 1] < cfg.stop_eigenvalue:
        break
      gaps.append(w[i - 1] / (w[i] + so.EPS) if ratio else (w[i - 1] - w[i]) / wmax)
  else:
    for i in range(1, end - 1):
      gaps.append(w[i + 1] / (w[i] + so.EPS) if ratio else (w[i + 1] - w[i]) / wmax)
  gaps = np.sort(np.asarray(gaps))[::-1]
  if len(gaps) < 2:
    return 1.0
  return float((gaps[0] - gaps[1]) / abs(gaps[0]))
