// dist_plan_driver.cpp -- the exchange layout of the sharded products (libfastsparse_amd/csrc/fs_dist_plan.h) behind a text
// protocol, for tests/test_dist_plan.py: plain C++17, no HIP, built with -fsanitize=address,undefined.
// stdin: one plan per line -- n k np, then bounds[n + 1], then cut[r][0 .. np] rank after rank.
// stdout: `case` and one `key v1 .. vn` line per output.
#include <iostream>
#include <vector>

#include "fs_dist_plan.h"

template <typename V>
static void put(const char *key, const V &v)
{
  std::cout << key;
  for (const auto &x : v) std::cout << ' ' << (long long)x;
  std::cout << '\n';
}

int main()
{
  int n, k, np;
  while (std::cin >> n >> k >> np) {
    std::vector<int> bounds((size_t)n + 1);
    for (int &b : bounds) std::cin >> b;
    std::vector<std::vector<int>> cut((size_t)n, std::vector<int>((size_t)np + 1));
    for (std::vector<int> &c : cut)
      for (int &v : c) std::cin >> v;
    const fs::ExchangePlan P = fs::plan_exchange(n, k, bounds, cut);
    std::cout << "case\n";
    put("scalars", std::vector<long long>{P.n, P.k, P.np, P.real, P.max_rows, P.nseg, P.nseg1, P.max_seg, P.pad_rows, P.local_rows, P.window_rows,
                                          fs::most_busy_parts(P.cut), (long long)(P.whole_shard_table(P.table.data()) - P.table.data())});
    put("maxc", P.maxc);
    put("off", P.off);
    put("table", P.table);
    std::vector<int> flat;
    for (const std::vector<int> &c : P.cut) flat.insert(flat.end(), c.begin(), c.end());
    put("cut", flat);
  }
  return 0;
}
