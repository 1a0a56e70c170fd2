// fs_pcgn_plan.h -- when fs_pcgn / fs_pcgn_lambdas under option "pcgn_compact" move their live columns into a narrower panel, as
// plain functions: the live masks the host learns in, the widths and the segments out.  No HIP here: this header compiles with
// a plain C++17 compiler, so the schedule runs on the host alone (tests/pcgn_plan_driver.cpp, tests/test_pcgn_plan.py, modelled in
// tests/_pcgn_plan_model.py).  include/fastsparse_hip.h states the rule under fs_pcgn; this is its one implementation: the solve
// (fs_cg.hip) drives a PcgnSchedule with the masks it reads, pcgn_plan drives the same object with masks made from counts.
#pragma once

#include <vector>

namespace fs {

// the widths a solve may run at: where the k-column products change price
constexpr int kPcgnRungs[] = {1, 2, 4, 8, 16, 32};

// W(L): the smallest rung that holds L columns (L in 1..32)
inline int pcgn_rung(int L)
{
  for (int w : kPcgnRungs)
    if (w >= L) return w;
  return 32;
}

inline int pcgn_popcount(unsigned m)
{
  int n = 0;
  for (; m; m &= m - 1u) ++n;
  return n;
}

inline unsigned pcgn_all_columns(int k) { return k < 32 ? (1u << k) - 1u : ~0u; }

// a run of iterations at one width: `first` is its first iteration, `mask` the ORIGINAL columns its panel holds (in increasing
// order, padding behind them)
struct PcgnSegment { int first, width; unsigned mask; };

// `usable`: bit w set for every rung w < k the solve may narrow to (rungs are powers of two: w is its own bit)
struct PcgnSchedule {
  int k, w;
  unsigned usable;
  std::vector<PcgnSegment> segs;
  PcgnSchedule(int k_, unsigned usable_) : k(k_), w(k_), usable(usable_), segs{{0, k_, pcgn_all_columns(k_)}} { segs.reserve(8); }

  // before iteration n is enqueued, with m = the live mask the host knows then (original numbering; never empty): the width to
  // repack to -- the narrowest usable rung w' with W(popcount(m)) <= w' < w -- or 0: nothing moves
  int before_iteration(int n, unsigned m)
  {
    const int need = pcgn_rung(pcgn_popcount(m));
    int to = 0;
    for (int v : kPcgnRungs)
      if (!to && v >= need && v < w && (usable & (unsigned)v) != 0u) to = v;
    if (!to) return 0;
    if (segs.back().first == n) segs.back() = PcgnSegment{n, to, m};     // (n = 0: the full-width segment never ran)
    else segs.push_back(PcgnSegment{n, to, m});
    w = to;
    return to;
  }
  // the host has learnt that the solve was done before iteration n: a repack enqueued with that iteration did nothing on the
  // device, like the iteration's other kernels, and is no segment
  void not_run(int n)
  {
    if (segs.size() > 1 && segs.back().first == n) {
      segs.pop_back();
      w = segs.back().width;
    }
  }
};

// The schedule of a solve from its outcome.  count[j]: column j's final count; frozen0[j] != 0: column j was frozen by the start
// kernels; cap: the iteration cap (>= 1).  Column j is live after iteration i iff it was live at the start and i < count[j] (a
// column that converges does so in iteration count[j]; one still live at the cap has count = cap).  m_0 = m_1 = the mask after the
// start, m_n = the mask after iteration n - 2: what the host, one iteration behind, has in hand when it enqueues iteration n
inline std::vector<PcgnSegment> pcgn_plan(int k, unsigned usable, const int *count, const int *frozen0, int cap)
{
  PcgnSchedule S(k, usable);
  unsigned m0 = 0u;
  for (int j = 0; j < k; ++j)
    if (!frozen0[j]) m0 |= 1u << j;
  auto after = [&](int i) {
    unsigned m = 0u;
    for (int j = 0; j < k; ++j)
      if (((m0 >> j) & 1u) != 0u && i < count[j]) m |= 1u << j;
    return m;
  };
  if (m0 == 0u) return S.segs;                               // done before the first iteration: nothing is enqueued
  for (int n = 0; n < cap; ++n) {
    S.before_iteration(n, n < 2 ? m0 : after(n - 2));
    if (n >= 1 && after(n - 1) == 0u) {                      // the flags of iteration n - 1 arrive behind iteration n: it did not run
      S.not_run(n);
      break;
    }
  }
  return S.segs;
}

}  // namespace fs
