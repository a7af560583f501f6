// ahc_tree_cut (spectralcluster_amd/csrc/ahc_tree.cpp) is called from several host threads at
// once by the stream pool.  This program cuts the same seeded merge lists once on one thread and
// then on several threads concurrently, and compares the labels.  Plain host code, meant to be
// built with the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       -I spectralcluster_amd/csrc tests/probes/ahc_tree_threads.cpp \
//       spectralcluster_amd/csrc/ahc_tree.cpp -o ahc_tree_threads
// Exit status 0 and "ok" on success.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <random>
#include <thread>
#include <vector>

#include "ahc_tree.h"

namespace {

struct Case {
  int n = 0, n_clusters = 0;
  double threshold = 0.0;
  std::vector<double> Z;
  std::vector<int64_t> want;
};

// A merge list in the nearest-neighbour chain's format: slots x < y, slot y keeps the cluster.
// Heights come from a small set, so the stable sort has ties to keep in order, and they are not
// monotone in merge order (the chain does not produce them sorted either).
Case make_case(uint32_t seed) {
  std::mt19937 rng(seed);
  Case c;
  const int sizes[] = {2, 3, 25, 64, 65, 129, 600, 1025};
  c.n = sizes[seed % 8];
  std::vector<int> alive(c.n), count(c.n, 1);
  for (int i = 0; i < c.n; ++i) alive[i] = i;
  c.Z.resize((size_t)(c.n - 1) * 4);
  for (int k = 0; k < c.n - 1; ++k) {
    const int a = (int)(rng() % alive.size());
    int b = (int)(rng() % (alive.size() - 1));
    if (b >= a) ++b;
    const int x = alive[a] < alive[b] ? alive[a] : alive[b];
    const int y = alive[a] < alive[b] ? alive[b] : alive[a];
    c.Z[(size_t)k * 4 + 0] = x;
    c.Z[(size_t)k * 4 + 1] = y;
    c.Z[(size_t)k * 4 + 2] = (double)(rng() % 17) / 16.0;
    c.Z[(size_t)k * 4 + 3] = count[x] + count[y];
    count[y] += count[x];
    alive.erase(alive.begin() + (alive[a] == x ? a : b));
  }
  if (seed % 3 == 0) {
    c.n_clusters = 0;  // distance_threshold mode
    c.threshold = (double)(rng() % 17) / 16.0;
  } else {
    c.n_clusters = 1 + (int)(rng() % c.n);
  }
  return c;
}

}  // namespace

int main() {
  const int kCases = 96, kThreads = 8, kRounds = 4;
  std::vector<Case> cases(kCases);
  for (int i = 0; i < kCases; ++i) {
    cases[i] = make_case(1000u + (uint32_t)i);
    Case& c = cases[i];
    c.want.assign(c.n, -1);
    const int k = sc::ahc_tree_cut(c.Z.data(), c.n, c.n_clusters, c.threshold, c.want.data());
    // every row labelled, every label in range, every label used
    std::vector<char> used(k, 0);
    for (int64_t v : c.want) {
      if (v < 0 || v >= k) {
        std::printf("case %d: label %lld outside 0..%d\n", i, (long long)v, k - 1);
        return 1;
      }
      used[v] = 1;
    }
    for (char u : used)
      if (!u) {
        std::printf("case %d: an empty cluster\n", i);
        return 1;
      }
    if (c.n_clusters > 0 && k != c.n_clusters) {
      std::printf("case %d: %d clusters, asked for %d\n", i, k, c.n_clusters);
      return 1;
    }
  }
  std::atomic<int> next{0}, bad{0};
  std::vector<std::thread> threads;
  for (int t = 0; t < kThreads; ++t)
    threads.emplace_back([&] {
      std::vector<int64_t> got;
      for (;;) {
        const int item = next.fetch_add(1);
        if (item >= kCases * kRounds) return;
        const Case& c = cases[item % kCases];
        got.assign(c.n, -1);
        sc::ahc_tree_cut(c.Z.data(), c.n, c.n_clusters, c.threshold, got.data());
        if (got != c.want) bad.fetch_add(1);
      }
    });
  for (std::thread& t : threads) t.join();
  if (bad.load() != 0) {
    std::printf("%d of %d concurrent cuts differ from the single-threaded run\n", bad.load(),
                kCases * kRounds);
    return 1;
  }
  std::printf("ok: %d cuts on %d threads equal the single-threaded labels\n", kCases * kRounds,
              kThreads);
  return 0;
}
