// Tree bookkeeping of the agglomerative clustering on the host (ahc_tree.h): O(n log n) scalar
// work on the n - 1 merges the device's nearest-neighbour chain produced.
#include "ahc_tree.h"

#include <algorithm>
#include <array>
#include <cstddef>
#include <utility>
#include <vector>

namespace sc {
namespace {
// CPython heapq (Lib/heapq.py) on ints: sklearn's _hc_cut enumerates the heap ARRAY, so
// the exact sift order defines the label numbering.
void heap_siftdown(std::vector<long long>& heap, size_t startpos, size_t pos) {
  const long long newitem = heap[pos];
  while (pos > startpos) {
    const size_t parentpos = (pos - 1) >> 1;
    const long long parent = heap[parentpos];
    if (newitem < parent) {
      heap[pos] = parent;
      pos = parentpos;
      continue;
    }
    break;
  }
  heap[pos] = newitem;
}
void heap_siftup(std::vector<long long>& heap, size_t pos) {
  const size_t endpos = heap.size(), startpos = pos;
  const long long newitem = heap[pos];
  size_t childpos = 2 * pos + 1;
  while (childpos < endpos) {
    const size_t rightpos = childpos + 1;
    if (rightpos < endpos && !(heap[childpos] < heap[rightpos])) childpos = rightpos;
    heap[pos] = heap[childpos];
    pos = childpos;
    childpos = 2 * pos + 1;
  }
  heap[pos] = newitem;
  heap_siftdown(heap, startpos, pos);
}
void heap_push(std::vector<long long>& heap, long long item) {
  heap.push_back(item);
  heap_siftdown(heap, 0, heap.size() - 1);
}
void heap_pushpop(std::vector<long long>& heap, long long item) {
  if (!heap.empty() && heap[0] < item) {
    std::swap(item, heap[0]);
    heap_siftup(heap, 0);
  }
}
}  // namespace

int ahc_tree_cut(const double* Z, int n, int n_clusters, double distance_threshold,
                 int64_t* labels) {
  // ---- scipy: stable sort by height, union-find relabelling (hierarchy.pyx `label`)
  std::vector<int> order(n - 1);
  for (int i = 0; i < n - 1; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return Z[(size_t)a * 4 + 2] < Z[(size_t)b * 4 + 2]; });
  std::vector<int> parent(2 * (size_t)n - 1);
  for (size_t i = 0; i < parent.size(); ++i) parent[i] = (int)i;
  auto find = [&](int v) {
    int r = v;
    while (parent[r] != r) r = parent[r];
    while (parent[v] != r) {
      const int next = parent[v];
      parent[v] = r;
      v = next;
    }
    return r;
  };
  std::vector<std::array<long long, 2>> children(n - 1);
  std::vector<double> heights(n - 1);
  int next_label = n;
  for (int i = 0; i < n - 1; ++i) {
    const int m = order[i];
    const int xr = find((int)Z[(size_t)m * 4]), yr = find((int)Z[(size_t)m * 4 + 1]);
    children[i] = {std::min(xr, yr), std::max(xr, yr)};
    heights[i] = Z[(size_t)m * 4 + 2];
    parent[xr] = next_label;
    parent[yr] = next_label;
    ++next_label;
  }
  // ---- sklearn: number of clusters, then _hc_cut
  int k = n_clusters;
  if (k == 0) {  // distance_threshold mode
    k = 1;
    for (int i = 0; i < n - 1; ++i) k += heights[i] >= distance_threshold;
  }
  std::vector<long long> nodes;
  nodes.push_back(-(std::max(children[n - 2][0], children[n - 2][1]) + 1));
  for (int it = 0; it < k - 1; ++it) {
    const auto c = children[(size_t)(-nodes[0] - n)];
    heap_push(nodes, -c[0]);
    heap_pushpop(nodes, -c[1]);
  }
  std::vector<long long> stack;
  for (size_t i = 0; i < nodes.size(); ++i) {
    stack.assign(1, -nodes[i]);
    while (!stack.empty()) {
      const long long v = stack.back();
      stack.pop_back();
      if (v < n) {
        labels[v] = (int64_t)i;
      } else {
        stack.push_back(children[(size_t)(v - n)][0]);
        stack.push_back(children[(size_t)(v - n)][1]);
      }
    }
  }
  return k;
}

}  // namespace sc
