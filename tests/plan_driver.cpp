// plan_driver.cpp -- the host planners of the copy builders (libfastsparse_amd/csrc/fs_plan.h) behind a text protocol, for
// tests/test_format_plans.py: plain C++17, no HIP, built with -fsanitize=address,undefined.
// stdin: one command per planner call -- its name, its scalar arguments, then its vectors as `n v1 .. vn`.
// stdout: `case <name>` and one `key v1 .. vn` line per output.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "fs_plan.h"

using namespace fs;

template <typename T>
static std::vector<T> read_vec()
{
  size_t n = 0;
  std::cin >> n;
  std::vector<T> v(n);
  for (T &x : v) std::cin >> x;
  return v;
}

template <typename V>
static void put(const char *key, const V &v)
{
  std::cout << key;
  for (const auto &x : v) std::cout << ' ' << (long long)x;
  std::cout << '\n';
}

int main()
{
  std::string cmd;
  while (std::cin >> cmd) {
    std::cout << "case " << cmd << '\n';
    if (cmd == "consts") {
      put("consts", std::vector<int>{kTiledItem, kTiledRowsMax, kTiledColBits, kLdsxRows, kLdsxCols, kBinCols, kBinRowsMax, kBinColsBig,
                                     kBinRowsBig, kBinBigRunEntries, kBinGroup, kLongOwners});
    } else if (cmd == "tiled_rows") {
      int nvrow, slots, rows_max, ldsx, tile_rows;
      std::cin >> nvrow >> slots >> rows_max >> ldsx >> tile_rows;
      put("R", std::vector<int>{plan_tiled_rows(nvrow, slots, rows_max, ldsx != 0, tile_rows)});
    } else if (cmd == "tiled_panels") {
      int nvrow, R, virt, split;
      long long nnz;
      std::cin >> nvrow >> R >> virt >> nnz >> split;
      const std::vector<int> vp = read_vec<int>();
      put("panel_row", plan_tiled_panels(nvrow, R, virt != 0, vp, nnz, split));
    } else if (cmd == "band_width") {
      int ncol, P, ldsx, tile_cols, W = 0, J = 0;
      long long nnz;
      std::cin >> ncol >> nnz >> P >> ldsx >> tile_cols;
      plan_band_width(ncol, nnz, P, ldsx != 0, tile_cols, &W, &J);
      put("WJ", std::vector<int>{W, J});
    } else if (cmd == "work_items") {
      int P, J, print;
      std::cin >> P >> J >> print;
      const std::vector<int> tp = read_vec<int>();
      std::vector<WorkItem> items;
      std::vector<int> item_ptr;
      cut_work_items(tp, P, J, items, item_ptr);
      put("nitems", std::vector<size_t>{items.size()});
      put("item_ptr", item_ptr);
      if (print) {
        std::vector<int> flat;
        for (const WorkItem &it : items) { flat.push_back(it.x); flat.push_back(it.y); flat.push_back(it.z); flat.push_back(it.w); }
        put("items", flat);
      }
    } else if (cmd == "ldsx_chunks") {
      int P, slots, plain;
      long long nitems;
      std::cin >> P >> slots >> plain >> nitems;
      const std::vector<int> item_ptr = read_vec<int>();
      std::vector<int> chunk_panel, chunk_item, chunk_ord;
      const bool shared = plan_ldsx_chunks(item_ptr, nitems, P, slots, plain != 0, chunk_panel, chunk_item, chunk_ord);
      put("shared", std::vector<int>{shared});
      put("chunk_panel", chunk_panel);
      put("chunk_item", chunk_item);
      put("chunk_ord", chunk_ord);
    } else if (cmd == "two_pass_geometry") {
      int nrow, ncol, kw, bin_rows, big_env;
      long long nnz;
      std::cin >> nrow >> ncol >> nnz >> kw >> bin_rows >> big_env;
      const TwoPassGeometry g = plan_two_pass_geometry(nrow, ncol, nnz, kw, bin_rows, big_env);
      put("geometry", std::vector<int>{g.big, g.bcols, g.rmax, g.ge, g.R});
    } else if (cmd == "two_pass_panels") {
      int nvrow, R, slots, min_panels, kw;
      long long nnz;
      double fill;
      std::cin >> nvrow >> nnz >> R >> slots >> fill >> min_panels >> kw;
      const std::vector<int> vp = read_vec<int>();
      put("panel_row", plan_two_pass_panels(vp, nvrow, nnz, R, slots, fill, min_panels, kw));
    } else if (cmd == "long_rows") {
      int cap_rows;
      std::cin >> cap_rows;
      const std::vector<int> flat = read_vec<int>();
      std::vector<RowLen> cand;
      for (size_t i = 0; i + 1 < flat.size(); i += 2) cand.push_back(RowLen{flat[i], flat[i + 1]});
      std::vector<int> rows, own_first;
      std::vector<unsigned char> owner_of;
      std::vector<int64_t> lptr;
      deal_long_rows(cand, cap_rows, rows, own_first, owner_of, lptr);
      put("rows", rows);
      put("own_first", own_first);
      put("owner_of", owner_of);
      put("lptr", lptr);
    } else if (cmd == "pad_segments") {
      int B;
      std::cin >> B;
      const std::vector<int64_t> hs = read_vec<int64_t>();
      std::vector<int64_t> hp, hsh;
      std::vector<unsigned> hseg;
      const bool ok = pad_long_segments(hs, B, hp, hseg, hsh);
      put("ok", std::vector<int>{ok});
      put("hp", hp);
      put("hseg", hseg);
      put("hsh", hsh);
    } else if (cmd == "generation_cuts") {
      int nunits, slots, nparts;
      std::cin >> nunits >> slots >> nparts;
      put("units", plan_generation_cuts(nunits, slots, nparts));
    } else {
      fprintf(stderr, "plan_driver: unknown command %s\n", cmd.c_str());
      return 2;
    }
    if (!std::cin) { fprintf(stderr, "plan_driver: short input in %s\n", cmd.c_str()); return 2; }
  }
  return 0;
}
