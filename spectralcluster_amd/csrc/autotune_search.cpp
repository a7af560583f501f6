// AutoTune's grid search over p_percentile (reference autotune.py:58-132), restated on the host
// so that a library batch can run it per utterance without the interpreter.  Host compiler; no
// device code.  The restatement is exact: the same grid doubles as np.linspace, the same
// "searched" set (exact double equality), the first strict minimum, the same narrowing.

#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/spectralcluster_amd.h"

namespace {
constexpr double kMinSearchStep = 1e-04;  // autotune.py: MIN_SEARCH_STEP
constexpr double kMaxGrid = 1 << 24;      // (a grid beyond this is a mistake, not a search)

// AutoTune.get_percentile_range: np.linspace(min, max, ceil((max - min) / step)).  numpy forms
// arange(num) * (delta / (num - 1)) + start (a product, then a sum), writes `stop` into the last
// element, and gives [start] for num == 1.  false: Python would raise (a non-finite or negative
// count).
bool percentile_range(double lo, double hi, double step, std::vector<double>* grid) {
  grid->clear();
  const double want = std::ceil((hi - lo) / step);
  if (!std::isfinite(want) || want < 0.0 || want > kMaxGrid) return false;
  const int num = (int)want;
  if (num == 0) return true;
  const double delta = hi - lo;
  grid->resize(num);
  if (num == 1) {
    (*grid)[0] = 0.0 * delta + lo;
    return true;
  }
  const double div = (double)(num - 1);
  const double stride = delta / div;
  for (int i = 0; i < num; ++i) {
    const double y = stride == 0.0 ? ((double)i / div) * delta : (double)i * stride;
    (*grid)[i] = y + lo;
  }
  (*grid)[num - 1] = hi;
  return true;
}
}  // namespace

extern "C" int sc_host_autotune_ratio(const sc_autotune* at, double p, double max_delta,
                                      double* ratio) {
  if (!at || !ratio) return SC_ERR_INVALID;
  if (at->proxy == SC_AUTOTUNE_PERCENTILE_SQRT_OVER_NME)
    *ratio = std::sqrt(1 - p) / max_delta;
  else if (at->proxy == SC_AUTOTUNE_PERCENTILE_OVER_NME)
    *ratio = (1 - p) / max_delta;
  else
    return SC_ERR_INVALID;
  return SC_OK;
}

extern "C" int sc_host_autotune_search(const sc_autotune* at, sc_autotune_evaluate evaluate_many,
                                       void* user, double* best_p, int* best_index,
                                       double* last_p, sc_autotune* narrowed) {
  if (!at || !evaluate_many) return SC_ERR_INVALID;
  if (at->proxy != SC_AUTOTUNE_PERCENTILE_OVER_NME &&
      at->proxy != SC_AUTOTUNE_PERCENTILE_SQRT_OVER_NME)
    return SC_ERR_INVALID;
  sc_autotune state = *at;
  std::vector<double> grid, next, searched, ps, ratios;
  std::vector<int> index;
  if (!percentile_range(state.p_min, state.p_max, state.step, &grid)) return SC_ERR_INVALID;
  bool have_best = false, evaluated_any = false;
  double win_p = 0.0, final_p = 0.0;
  int win_index = 0;
  for (int level = 0; level < state.levels; ++level) {
    double lowest = std::numeric_limits<double>::infinity();
    ps.clear();
    index.clear();
    for (int i = 0; i < (int)grid.size(); ++i) {
      bool seen = false;
      for (double q : searched) seen = seen || q == grid[i];
      if (!seen) {
        ps.push_back(grid[i]);
        index.push_back(i);
      }
    }
    ratios.assign(ps.size(), std::numeric_limits<double>::quiet_NaN());
    if (!ps.empty()) {
      const int rc = evaluate_many(ps.data(), (int)ps.size(), ratios.data(), user);
      if (rc != SC_OK) return rc;
      evaluated_any = true;
      final_p = ps.back();
    }
    for (size_t j = 0; j < ps.size(); ++j) {
      searched.push_back(ps[j]);
      if (ratios[j] < lowest) {  // the first strict minimum of the level wins
        lowest = ratios[j];
        win_p = ps[j];
        win_index = index[j];
        have_best = true;
      }
    }
    const int len = (int)grid.size();
    if (len == 0 || len == 1 || state.step < kMinSearchStep) break;
    if (!have_best) return SC_ERR_INVALID;  // (no finite ratio yet: Python fails here as well)
    const int reach = len / 8 > 2 ? len / 8 : 2;
    const int low = win_index - reach > 0 ? win_index - reach : 0;
    const int high = win_index + reach < len - 1 ? win_index + reach : len - 1;
    if (low > len - 1) return SC_ERR_INVALID;  // (a winner kept from a longer, earlier grid)
    state.p_min = grid[low];
    state.p_max = grid[high];
    state.step = state.step / 2;
    if (!percentile_range(state.p_min, state.p_max, state.step, &next)) return SC_ERR_INVALID;
    grid.swap(next);
  }
  if (!have_best || !evaluated_any) return SC_ERR_INVALID;
  if (best_p) *best_p = win_p;
  if (best_index) *best_index = win_index;
  if (last_p) *last_p = final_p;
  if (narrowed) *narrowed = state;
  return SC_OK;
}
