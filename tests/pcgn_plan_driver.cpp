// pcgn_plan_driver.cpp -- the narrowing schedule of fs_pcgn / fs_pcgn_lambdas under option "pcgn_compact"
// (libfastsparse_amd/csrc/fs_pcgn_plan.h) behind a text protocol, for tests/test_pcgn_plan.py: plain C++17, no HIP, built with
// -fsanitize=address,undefined.
// stdin: one solve per line -- k usable cap, then count[k], then frozen0[k] (usable: bit w set for every usable rung w < k).
// stdout: `case`, then `segments first width mask ...` (three numbers per segment) and `rungs W(1) .. W(k)`.
#include <iostream>
#include <vector>

#include "fs_pcgn_plan.h"

int main()
{
  int k, cap;
  unsigned usable;
  while (std::cin >> k >> usable >> cap) {
    std::vector<int> count((size_t)k), frozen0((size_t)k);
    for (int &c : count) std::cin >> c;
    for (int &f : frozen0) std::cin >> f;
    const std::vector<fs::PcgnSegment> segs = fs::pcgn_plan(k, usable, count.data(), frozen0.data(), cap);
    std::cout << "case\nsegments";
    for (const fs::PcgnSegment &s : segs) std::cout << ' ' << s.first << ' ' << s.width << ' ' << (unsigned long long)s.mask;
    std::cout << "\nrungs";
    for (int L = 1; L <= k; ++L) std::cout << ' ' << fs::pcgn_rung(L);
    std::cout << '\n';
  }
  return 0;
}
