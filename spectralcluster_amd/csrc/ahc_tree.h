// Host half of the agglomerative clustering (ahc.hip has the device half): from the merge list
// of the nearest-neighbour chain to sklearn's labels.  scipy sorts the merges by height (stable)
// and relabels them with a union-find (hierarchy.pyx `label`); sklearn cuts the tree with a heap
// of node ids (_hc_cut), and the heap ARRAY's order is the label numbering.
// Host-only, no HIP: built with the host compiler.  Reentrant -- every call works on its own
// vectors, so the trees of a stream pool's sessions are cut on several threads at once.
#ifndef SPECTRALCLUSTER_AMD_AHC_TREE_H_
#define SPECTRALCLUSTER_AMD_AHC_TREE_H_

#include <stdint.h>

namespace sc {

// Z: (n - 1) x 4 doubles (slot x, slot y, height, size) in merge order, as k_ahc_nn_chain leaves
// them; n >= 2.  n_clusters > 0: that many clusters; n_clusters == 0: as many as
// distance_threshold leaves (merges at or above it are undone).  labels: n values, numbered as
// sklearn.cluster.AgglomerativeClustering numbers them.  Returns the cluster count.
int ahc_tree_cut(const double* Z, int n, int n_clusters, double distance_threshold,
                 int64_t* labels);

}  // namespace sc

#endif  // SPECTRALCLUSTER_AMD_AHC_TREE_H_
