// fs_dist_plan.h -- the layout of the exchange of a row-sharded product (fs_dist.hip) as a plain function: the ranks' row
// bounds and the cuts of their local products in, the padded regions, the unpack tables and the buffer sizes out.  No HIP
// here: this header compiles with a plain C++17 compiler, so the arithmetic that decides which send window runs past a
// shard's last row and where rank r's rows land in the padded buffer runs on the host alone (tests/dist_plan_driver.cpp,
// tests/test_dist_plan.py, modelled in tests/_dist_plan_model.py).  One plan serves every k: counts are kept in ROWS, the
// tables are in doubles (rows x k), which is what fs_copy_segments reads.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace fs {

// Rank r owns rows [bounds[r], bounds[r + 1]) and finishes its local rows [cut[r][p], cut[r][p + 1]) in part p.
//   overlapped layout   part p is ONE all-gather of maxc[p] * k doubles per rank -- from local + cut[r][p] * k (a window that
//                       may run past the shard's last row) into pad + off[p] * k: rank r's rows of part p arrive at row
//                       off[p] + r * maxc[p];
//   whole-shard layout  ONE all-gather of max_rows * k doubles per rank: rank r's rows arrive at row r * max_rows.
struct ExchangePlan {
  int n = 0, k = 1, np = 0;
  std::vector<std::vector<int>> cut;    // [rank][part]: np + 1 row cuts of the local product
  std::vector<int> maxc;                // [part]: the most rows any rank finishes in the part
  std::vector<int64_t> off;             // [part]: first ROW of the part's region of the padded buffer; off[np]: rows of all regions
  bool real = false;                    // some rank finishes rows in more than one part: the overlapped exchange has something to hide
  int max_rows = 0;                     // the tallest shard
  // host image of the unpack table: [dst .. src .. cnt] of the overlapped layout (nseg segments), then [dst .. src .. cnt] of
  // the whole-shard layout (nseg1 segments), in doubles
  std::vector<int64_t> table;
  int nseg = 0, nseg1 = 0;
  int64_t max_seg = 0;                  // the longest segment of the overlapped layout, in doubles
  // what the buffers need, in rows (x k doubles; the allocations add one element)
  int64_t pad_rows = 0;                 // padded receive buffer: either layout fits
  int64_t local_rows = 1;               // local output: a window of maxc[p] <= max_rows rows from any cut <= max_rows stays inside
  int64_t window_rows = 0;              // whole-shard send window

  const int64_t *whole_shard_table(const int64_t *per_part_table) const { return per_part_table + 3 * (size_t)nseg; }
};

// in how many parts the busiest rank finishes rows
inline int most_busy_parts(const std::vector<std::vector<int>> &cut)
{
  int most = 0;
  for (const std::vector<int> &c : cut) {
    int busy = 0;
    for (size_t p = 0; p + 1 < c.size(); ++p) busy += c[p + 1] > c[p];
    most = std::max(most, busy);
  }
  return most;
}

// cut: n vectors of np + 1 cuts each (all zero for a rank without rows)
inline ExchangePlan plan_exchange(int n, int k, const std::vector<int> &bounds, std::vector<std::vector<int>> cut)
{
  ExchangePlan P;
  P.n = n;
  P.k = k;
  P.np = cut.empty() ? 0 : (int)cut[0].size() - 1;
  P.cut = std::move(cut);
  P.real = most_busy_parts(P.cut) > 1;
  const int np = P.np;
  auto rows = [&](int r, int p) { return P.cut[(size_t)r][(size_t)p + 1] - P.cut[(size_t)r][(size_t)p]; };
  for (int r = 0; r < n; ++r) P.max_rows = std::max(P.max_rows, bounds[(size_t)r + 1] - bounds[(size_t)r]);
  P.maxc.assign((size_t)np, 0);
  P.off.assign((size_t)np + 1, 0);
  for (int p = 0; p < np; ++p) {
    for (int r = 0; r < n; ++r) P.maxc[(size_t)p] = std::max(P.maxc[(size_t)p], rows(r, p));
    P.off[(size_t)p + 1] = P.off[(size_t)p] + (int64_t)n * P.maxc[(size_t)p];
  }
  std::vector<int64_t> dst, src, cnt;
  auto append = [&] {
    P.table.insert(P.table.end(), dst.begin(), dst.end());
    P.table.insert(P.table.end(), src.begin(), src.end());
    P.table.insert(P.table.end(), cnt.begin(), cnt.end());
    const int nseg = (int)cnt.size();
    dst.clear(); src.clear(); cnt.clear();
    return nseg;
  };
  for (int p = 0; p < np; ++p)
    for (int r = 0; r < n; ++r) {
      const int64_t c = rows(r, p);
      if (!c) continue;
      dst.push_back(((int64_t)bounds[(size_t)r] + P.cut[(size_t)r][(size_t)p]) * k);
      src.push_back((P.off[(size_t)p] + (int64_t)r * P.maxc[(size_t)p]) * k);
      cnt.push_back(c * k);
      P.max_seg = std::max<int64_t>(P.max_seg, c * k);
    }
  P.nseg = append();
  for (int r = 0; r < n; ++r) {
    const int64_t c = bounds[(size_t)r + 1] - bounds[(size_t)r];
    if (!c) continue;
    dst.push_back((int64_t)bounds[(size_t)r] * k);
    src.push_back((int64_t)r * P.max_rows * k);
    cnt.push_back(c * k);
  }
  P.nseg1 = append();
  P.pad_rows = std::max<int64_t>(P.off[(size_t)np], (int64_t)n * P.max_rows);
  P.local_rows = 2 * (int64_t)P.max_rows + 1;
  P.window_rows = P.max_rows;
  return P;
}

}  // namespace fs
