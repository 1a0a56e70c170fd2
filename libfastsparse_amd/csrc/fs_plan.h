// fs_plan.h -- the host decisions of the copy builders (fs_copies.hip) as plain functions: numbers and std::vectors in,
// std::vectors out.  No HIP here: this header compiles with a plain C++17 compiler, so every decision that shapes a
// product -- panels, band width, work items, chunks and their launch order, the two-pass panels, the deal of long rows to
// their owners -- runs on the host alone (tests/plan_driver.cpp, tests/test_format_plans.py, modelled in
// tests/_plan_model.py).  The cost estimates that rule a copy out in auto mode are here as predicates, with the
// measurements their constants come from.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "fs_geometry.h"

namespace fs {

struct WorkItem { int x, y, z, w; };    // {first entry, count, band, 0}: the int4 of TiledCsr::items
struct RowLen { int x, y; };            // {row, entries}: the int2 of a long-row candidate

// ---- L2-tiled / LDS-staged copy ---------------------------------------------------------------------------------------
// pays when x does not fit the 32 KiB L1 of a CU many times over ...
// (measured, config-2 rows and non-zeros: x of 0.5-2 MB 0.75-0.82 ms tiled vs 0.92 ms streaming -- narrow
// bands are L1 resident; x of 4-80 MB 0.70-1.06 ms vs 1.07-2.99 ms; x of 64 KB 1.3 ms vs 0.8 ms)
inline bool tiled_too_small(int64_t x_bytes, int64_t nnz) { return x_bytes <= (256 << 10) || nnz < (4 << 20); }

// panels: at most R virtual rows (tile_rows > 0 forces R)
inline int plan_tiled_rows(int nvrow, int slots, int rows_max, bool ldsx, int tile_rows)
{
  int R = tile_rows;
  if (R <= 0) {
    const int64_t g = ((int64_t)nvrow + (int64_t)slots * rows_max - 1) / ((int64_t)slots * rows_max);
    R = (int)(((int64_t)nvrow + slots * g - 1) / (slots * g));
    if (R < 256) R = nvrow < 256 ? nvrow : 256;
    // few rows: full-height panels (dense tiles), cut into chunks below so that every CU still has work
    // (as equal as the row count allows: a remainder panel of a few hundred rows still sweeps every band -- 1 M rows under a limit
    // of 14 272 rows left one of 960 rows whose single chunk of 4 883 nearly empty phases took as long as everything else
    // together: config 3 transposed 0.75 -> 1.10 ms, profiles/r03_c3_kernel_variants_and_panel_cliff.jsonl)
    if (ldsx && (int64_t)nvrow < (int64_t)slots * rows_max / 2) {
      const int np = (int)(((int64_t)nvrow + rows_max - 1) / rows_max);
      R = (int)(((int64_t)nvrow + np - 1) / (np > 0 ? np : 1));
    }
  }
  if (R > rows_max) R = rows_max;
  return R;
}

// first virtual row of every panel and nvrow behind them (P + 1 values).  With cut rows (vp = the nvrow + 1 entry offsets
// of the virtual rows), panels of EQUAL non-zero count (0.8x what R average rows hold, so that nearly every panel is bounded
// by non-zeros, not by rows): the band sweep stays in step only if all workgroups of a generation carry the same work
inline std::vector<int> plan_tiled_panels(int nvrow, int R, bool virt, const std::vector<int> &vp, int64_t nnz, int split)
{
  std::vector<int> panel_row;
  if (!virt) {
    for (int r = 0; r < nvrow; r += R) panel_row.push_back(r);
  } else {
    const int64_t cap = (int64_t)(0.8 * (double)nnz * R / nvrow) + split;
    for (int r = 0; r < nvrow;) {
      panel_row.push_back(r);
      int e = (r + R < nvrow) ? r + R : nvrow;
      if ((int64_t)vp[e] - vp[r] > cap) {  // largest e with nnz(r..e) <= cap, at least one row
        e = (int)(std::upper_bound(vp.begin() + r + 1, vp.begin() + e + 1, (int)(vp[r] + cap)) - vp.begin()) - 1;
        if (e <= r) e = r + 1;
      }
      r = e;
    }
  }
  panel_row.push_back(nvrow);
  return panel_row;
}

// band width: tiles of about 0.9 work items on average, at most 2 MiB of x (L2-resident bands) or one LDS slice
// (LDS-staged kernel); tile_cols > 0 forces W
inline void plan_band_width(int ncol, int64_t nnz, int P, bool ldsx, int tile_cols, int *W_out, int *J_out)
{
  const int w_max = ldsx ? kLdsxCols : (1 << kTiledColBits);
  int W = tile_cols;
  if (W <= 0) {
    // (LDS-staged: 0.95 -- a slice costs its 16 KiB whatever the tile holds; config 3 transposed 0.777 -> 0.752 ms with
    // 2048-column slices instead of the 1904 that 0.85 gave, 1800 / 1600: 0.80 / 0.86)
    double w = (ldsx ? 0.95 : 0.9) * kTiledItem * (double)ncol * P / (double)nnz;
    if (w < (ldsx ? 256 : 4096)) w = ldsx ? 256 : 4096;
    if (w > w_max) w = w_max;
    W = (int)w;
  }
  if (W > w_max) W = w_max;
  if (W > ncol) W = ncol;
  if (ldsx && (W & 1) && W < w_max) ++W;   // slices are loaded two columns per thread
  *W_out = W;
  *J_out = (ncol + W - 1) / W;
}

// every tile costs one barrier phase and one slice of x from L2: worth it only when the tiles are reasonably
// full (config 3, 10 M x 1 M x 64 per row: 1 700 entries per tile; config 2: 43).  Beyond that the choice is
// measured (choose_copy).  With the DMA kernel the crossover against the L2-tiled kernel lies near 500 entries per
// tile (10 M rows x 16: 786 K columns, 543 per tile: 0.64 against 0.71 ms; 1 M columns, 407: 0.79 against 0.74)
inline bool ldsx_tiles_thin(int64_t nnz, int64_t ntiles) { return (double)nnz / ntiles < 450.0; }

// Structured matrices (banded, block-diagonal: x close to the diagonal) fill few of a panel's tiles, and those densely:
// the bands a sample of panels really touches (hc[2i] = bands, hc[2i + 1] = entries of sampled panel i) are counted before
// giving up on the average over ALL tiles
inline bool ldsx_sample_thin(const std::vector<int> &hc)
{
  double tiles = 0, entries = 0;
  for (size_t i = 0; i + 1 < hc.size(); i += 2) { tiles += hc[i]; entries += hc[i + 1]; }
  return tiles < 1 || entries / tiles < 450.0;
}

// tiles must not be hopelessly thin, and re-reading x once per generation of resident workgroups must
// cost less than the L2 misses it saves.  Measured: tiled ~150 G entries/s; one generation's sweep of x
// costs ~x_bytes / 2.7 TB/s (the XCDs sweep in step, so a band leaves HBM once and the other seven L2s are
// filled from the Infinity Cache: 10 M rows x 16, x of 80 / 160 / 320 / 800 MB: 1.06 / 1.22 / 1.52 / 1.96 ms);
// streaming kernel ~172 G entries/s while x stays L2 resident, ~53 G entries/s once every gather misses.
inline bool tiled_hopeless(int64_t nnz, int64_t ntiles, int P, int slots, int64_t x_bytes)
{
  if ((double)nnz / ntiles < 256.0) return true;
  const double gens = (double)((P + slots - 1) / slots);
  const double t_tiled = (double)nnz / 150e9 + gens * (double)x_bytes / 2.7e12;
  const double t_stream = (double)nnz / (x_bytes <= (3 << 20) ? 172e9 : 53e9);
  return t_tiled > 0.95 * t_stream;
}

// work items cut from the tile pointers (P * J + 1 ints): runs of at most kTiledItem entries of one tile; item_ptr[p] =
// first item of panel p (P + 1 values)
inline void cut_work_items(const std::vector<int> &tp, int P, int J, std::vector<WorkItem> &items, std::vector<int> &item_ptr)
{
  const int64_t ntiles = (int64_t)P * J;
  items.clear();
  item_ptr.assign((size_t)P + 1, 0);
  items.reserve((size_t)(tp[(size_t)ntiles] / kTiledItem + ntiles / 4 + 16));
  for (int p = 0; p < P; ++p) {
    item_ptr[p] = (int)items.size();
    for (int j = 0; j < J; ++j) {
      // 64-bit offsets: with nnz within 2 047 of INT_MAX `off += cap` wrapped around and this loop never ended
      // (caught by test_pattern_matrix_at_the_int32_limit: 270 GB of work items on the host)
      const int64_t a = tp[(size_t)p * J + j], b = tp[(size_t)p * J + j + 1];
      for (int64_t off = a; off < b; off += kTiledItem) {
        WorkItem it;
        it.x = (int)off; it.y = (int)((b - off < kTiledItem) ? b - off : kTiledItem); it.z = j; it.w = 0;
        items.push_back(it);
      }
    }
  }
  item_ptr[P] = (int)items.size();
}

// LDS-staged kernel, chunks: exactly `total` of them (a whole number of generations of resident workgroups: 264 equal
// chunks on 256 CUs take as long as 512) with entry counts as equal as the panels allow; a panel gets its share, at least
// one, cut at item boundaries.  Measured on config 3 transposed (66 panels): 1 / 2 / 4 / 8 chunks per CU 3.7 / 3.7 /
// 2.3 / 1.9 ms with rounded shares.
// (a chunk costs its PHASES: a work item takes about the same time whatever it holds, so panels are given chunks, and
// chunks are cut, by numbers of work items)
// Out, in launch order: chunk_panel (panel | bit 31 when the panel has several chunks), chunk_item (first, one past the last
// item), chunk_ord (ordinal inside the panel).  Returns whether some panel has more than one chunk.
inline bool plan_ldsx_chunks(const std::vector<int> &item_ptr, int64_t nitems, int P, int slots, bool plain_order,
                             std::vector<int> &chunk_panel, std::vector<int> &chunk_item, std::vector<int> &chunk_ord)
{
  bool shared = false;
  const int64_t total = (P >= slots) ? P : 8 * (int64_t)slots;
  std::vector<int64_t> nnz_p((size_t)P, 0);
  std::vector<int> k_p((size_t)P, 1);
  std::vector<std::pair<double, int>> frac;
  int64_t given = 0;
  for (int p = 0; p < P; ++p) {
    nnz_p[p] = item_ptr[p + 1] - item_ptr[p];
    const double share = (double)nnz_p[p] * (double)total / (double)(nitems == 0 ? 1 : nitems);
    const int cap = item_ptr[p + 1] - item_ptr[p] > 0 ? item_ptr[p + 1] - item_ptr[p] : 1;
    int k = (int)share;
    if (k < 1) k = 1;
    if (k > cap) k = cap;
    k_p[p] = k;
    given += k;
    if (k < cap) frac.push_back(std::make_pair(share - (double)(int)share, p));
  }
  std::sort(frac.begin(), frac.end(), [](const std::pair<double, int> &a, const std::pair<double, int> &b) {
    return a.first > b.first || (a.first == b.first && a.second < b.second);
  });
  for (size_t f = 0; f < frac.size() && given < total; ++f, ++given) ++k_p[frac[f].second];
  // chunk = (panel | shared flag, first item, one past the last item)
  struct Chunk { int panel, first, last, ordinal; };
  std::vector<Chunk> chunks;
  for (int p = 0; p < P; ++p) {
    const int i0 = item_ptr[p], i1 = item_ptr[p + 1], k = k_p[p];
    const int flag = k > 1 ? (int)0x80000000u : 0;
    if (k > 1) shared = true;
    int i = i0;
    int64_t done = 0;
    for (int c = 0; c < k; ++c) {
      const int first = i;
      const int64_t goal = nnz_p[p] * (c + 1) / k;
      while (i < i1 && (done < goal || c == k - 1)) { ++i; ++done; }
      chunks.push_back(Chunk{p | flag, first, i, c});
    }
  }
  // Launch order.  Workgroups that run together should sweep the SAME column bands, so that a band's slice of x
  // comes out of the XCD's L2 for all but the first of them: with several chunks per panel (few, long rows: config
  // 3 transposed, 66 panels x 31 chunks) the c-th chunks of all panels -- the same stretch of bands -- are launched
  // next to each other instead of panel by panel.  Blocks b and b + 8 share an XCD, so every XCD gets a share of
  // each stretch.  (Panel-major order read every slice from the Infinity Cache 66 times: 5.3 GB of slices against
  // 2.6 GB of entries, 1.84 ms; this order 1.06 ms.)
  // (second refinement: blocks b, b + 8, b + 16, ... land on the same XCD, so within a group of eight stretches the
  // order is panel-major with the stretch as the fastest index: an XCD then sees ONE stretch of bands for all panels
  // and is the only XCD that fetches its slices.  plain_order (FS_LDSX_ORDER=1) keeps the plain stretch-major order.)
  if (shared) {
    if (plain_order)
      std::stable_sort(chunks.begin(), chunks.end(), [](const Chunk &a, const Chunk &b) { return a.ordinal < b.ordinal; });
    else
      std::stable_sort(chunks.begin(), chunks.end(), [](const Chunk &a, const Chunk &b) {
        const int ga = a.ordinal >> 3, gb = b.ordinal >> 3;
        if (ga != gb) return ga < gb;
        const int pa = a.panel & 0x7fffffff, pb = b.panel & 0x7fffffff;
        if (pa != pb) return pa < pb;
        return (a.ordinal & 7) < (b.ordinal & 7);
      });
  }
  chunk_panel.clear(); chunk_item.clear(); chunk_ord.clear();
  for (const Chunk &c : chunks) {
    chunk_panel.push_back(c.panel);
    chunk_item.push_back(c.first);
    chunk_item.push_back(c.last);
    chunk_ord.push_back(c.ordinal);
  }
  return shared;
}

// ---- two-pass copy ------------------------------------------------------------------------------------------------------
struct TwoPassGeometry {
  bool big;    // short runs: the large bands and panels (kBinColsBig).  big_env (FS_BIN_BIG) 0 / 1 never / always, < 0 auto
  int bcols;   // columns per band: kw * 8 bytes of X per column in LDS
  int rmax;    // rows per panel: kw * 8 bytes of Y per row in LDS
  int ge;      // entries per group: a group of products is one 128-byte line
  int R;       // rows per panel asked for (bin_rows > 0 forces it), at most rmax
};

inline TwoPassGeometry plan_two_pass_geometry(int nrow, int ncol, int64_t nnz, int kw, int bin_rows, int big_env)
{
  TwoPassGeometry g;
  const double per_run = (double)nnz / ((double)((ncol + kBinCols - 1) / kBinCols) * (double)((nrow + kBinRowsMax - 1) / kBinRowsMax));
  g.big = kw == 1 && bin_rows == 0 && (big_env >= 0 ? big_env != 0 : per_run < kBinBigRunEntries);
  g.bcols = g.big ? kBinColsBig : kBinCols / kw;
  g.rmax = g.big ? kBinRowsBig : kBinRowsMax / kw;
  g.ge = kBinGroup / kw;
  g.R = bin_rows > 0 ? bin_rows : g.rmax;
  if (g.R > g.rmax) g.R = g.rmax;
  return g;
}

// panels of equal non-zero count, at most R rows: pass 2 runs one workgroup per panel and they all have to finish
// together; the count is a whole number of generations of resident workgroups.  vp = the nvrow + 1 entry offsets of the
// (virtual) rows; fill (FS_BIN_FILL / 100) = how full a panel of R rows is on average; P + 1 values out
inline std::vector<int> plan_two_pass_panels(const std::vector<int> &vp, int nvrow, int64_t nnz, int R, int slots, double fill,
                                             int min_panels, int kw)
{
  int64_t want = (int64_t)((double)nvrow / (fill * R)) + 1;
  if (want > slots) want = (want + slots - 1) / slots * slots;
  // fewer panels than CUs (a shard of 1-3 M rows: strong scaling cuts config 2 into such): pass 2 would leave most of the chip
  // idle, so the panels are made smaller until every CU has one (min_panels = FS_BIN_MIN_PANELS, 0 keeps the tall panels: A/B runs)
  if (min_panels && want < slots && (int64_t)nvrow >= (int64_t)slots * 256 && kw == 1) want = slots;
  std::vector<int> panel_row;
  {
    int r = 0;
    for (int64_t k = 1; k <= want && r < nvrow; ++k) {
      // the row boundary nearest to k/want of the non-zeros (so that rounding never adds up), then the row cap
      const int64_t goal = (int64_t)((double)nnz * (double)k / (double)want);
      int e = (int)(std::lower_bound(vp.begin() + r, vp.end(), goal,
                                     [](int a, int64_t b) { return (int64_t)a < b; }) - vp.begin());
      if (e > r && e <= nvrow && (int64_t)vp[e] - goal > goal - (int64_t)vp[e - 1] && e - 1 > r) --e;
      if (k == want || e > nvrow) e = nvrow;
      while (r < e) {
        panel_row.push_back(r);
        r = (e - r > R) ? r + R : e;
      }
    }
    if (panel_row.empty()) panel_row.push_back(0);
  }
  panel_row.push_back(nvrow);
  return panel_row;
}

// padding would dominate (a run is padded to whole groups: (ge - 1) / 2 entries on average)
inline bool two_pass_padding_dominates(int64_t nnz, int64_t nruns, int ge) { return (double)nnz / (double)nruns < 1.5 * ge; }

// two streaming passes (measured 4.6-5.0 TB/s) against what the other kernels reach on this shape; n = padded entries
inline bool two_pass_hopeless(int64_t n, bool valued, int B, int ncu, int bcols, int nvrow, int ncol, int64_t nnz)
{
  const double x_bytes = (double)ncol * 8;
  const double t_bin = ((double)n * (valued ? 28.5 : 20.5) + (double)(B + ncu) * bcols * 8 + (double)nvrow * 8) / 4.6e12;
  const double t_stream = (double)nnz / (x_bytes <= (3 << 20) ? 172e9 : 53e9);
  return t_bin > 0.95 * t_stream;   // hopeless; between the survivors choose_copy measures
}

// ---- long rows ----------------------------------------------------------------------------------------------------------
// The candidates' longest cap_rows rows are taken.  Owners: the rows, longest first, are dealt out to the kLongOwners waves
// in a snake (0 .. 15, 15 .. 0, ...), so that every owner carries about the same number of entries; inside an owner's block
// the rows ascend.  Long row index = position in the concatenation of the blocks: rows[i] its row, lptr its entry offsets
// (nlong + 1), own_first[w] the first index of owner w (kLongOwners + 1), owner_of[i] its owner.
inline void deal_long_rows(std::vector<RowLen> h, int cap_rows, std::vector<int> &rows, std::vector<int> &own_first,
                           std::vector<unsigned char> &owner_of, std::vector<int64_t> &lptr)
{
  std::sort(h.begin(), h.end(), [](const RowLen &a, const RowLen &b) { return a.y != b.y ? a.y > b.y : a.x < b.x; });
  if ((int)h.size() > cap_rows) h.resize((size_t)cap_rows);          // the longest ones
  const int nlong = (int)h.size();
  own_first.assign((size_t)kLongOwners + 1, 0);
  {
    std::vector<std::vector<RowLen>> blk((size_t)kLongOwners);
    for (int i = 0; i < nlong; ++i) {
      const int lap = i / kLongOwners, pos = i % kLongOwners;
      blk[(size_t)((lap & 1) ? kLongOwners - 1 - pos : pos)].push_back(h[(size_t)i]);
    }
    h.clear();
    for (int w = 0; w < kLongOwners; ++w) {
      std::sort(blk[(size_t)w].begin(), blk[(size_t)w].end(), [](const RowLen &a, const RowLen &b) { return a.x < b.x; });
      own_first[(size_t)w] = (int)h.size();
      h.insert(h.end(), blk[(size_t)w].begin(), blk[(size_t)w].end());
    }
    own_first[(size_t)kLongOwners] = (int)h.size();
  }
  owner_of.assign((size_t)nlong, 0);
  for (int w = 0; w < kLongOwners; ++w)
    for (int i = own_first[(size_t)w]; i < own_first[(size_t)w + 1]; ++i) owner_of[(size_t)i] = (unsigned char)w;
  rows.assign((size_t)nlong, 0);
  lptr.assign((size_t)nlong + 1, 0);
  for (int i = 0; i < nlong; ++i) { rows[(size_t)i] = h[(size_t)i].x; lptr[(size_t)i + 1] = lptr[(size_t)i] + h[(size_t)i].y; }
}

// worth a second kernel (and a second sweep over x: 8 bytes per column against 18 saved per entry)?  nl = their entries
inline bool long_rows_pay(int64_t nl, int64_t nnz, int ncol)
{
  return !((double)nl < 0.10 * (double)nnz || 18.0 * (double)nl < 16.0 * (double)ncol);
}

// the segments: (band, owner) in that order, each padded to an even count.  hs = first sorted entry of every segment
// (B * kLongOwners + 1); out: hp[b] = padded position of band b (B + 1), hseg = the segments' positions relative to their
// band (B * (kLongOwners + 1)), hsh[seg] = padded position - sorted position.  false: a band of 4 G entries: not this path
inline bool pad_long_segments(const std::vector<int64_t> &hs, int B, std::vector<int64_t> &hp, std::vector<unsigned> &hseg,
                              std::vector<int64_t> &hsh)
{
  const int64_t nseg = (int64_t)B * kLongOwners;
  hp.assign((size_t)B + 1, 0);
  hsh.assign((size_t)nseg + 1, 0);
  hseg.assign((size_t)B * (kLongOwners + 1), 0u);
  int64_t at = 0;                                 // padded position of the next segment
  for (int b = 0; b < B; ++b) {
    hp[(size_t)b] = at;
    for (int w = 0; w < kLongOwners; ++w) {
      const int64_t sg = (int64_t)b * kLongOwners + w;
      const int64_t c = hs[(size_t)sg + 1] - hs[(size_t)sg];
      hseg[(size_t)b * (kLongOwners + 1) + (size_t)w] = (unsigned)(at - hp[(size_t)b]);
      hsh[(size_t)sg] = at - hs[(size_t)sg];
      at += (c + 1) & ~(int64_t)1;
    }
    hseg[(size_t)b * (kLongOwners + 1) + (size_t)kLongOwners] = (unsigned)(at - hp[(size_t)b]);
    if (at - hp[(size_t)b] >= (1ll << 32)) return false;
  }
  hp[(size_t)B] = at;
  return true;
}

// ---- products in parts, products with host vectors --------------------------------------------------------------------------
// nunits workgroups (pass-2 panels, panels of a tiled copy), `slots` of them resident together (one per CU) and launches of one
// stream running one after the other: a part is a whole number of GENERATIONS of resident workgroups, so that the parts together
// take as many generations as the undivided launch.  4 parts of 192 panels on 256 CUs would take 4 generations where config 2's
// 768 panels take 3; config 3's 698 panels = 256 + 256 + 186 in eight ranges of 87 were measured at 2.42 ms per call against
// 1.87.  units[0 .. nparts]: part p is the workgroups [units[p], units[p + 1]); with fewer generations than parts the last
// parts are empty.  Whether to cut at all is the caller's question.
inline std::vector<int> plan_generation_cuts(int nunits, int slots, int nparts)
{
  const int gens = (int)(((int64_t)nunits + slots - 1) / slots);
  const int c = nparts < gens ? nparts : gens;
  std::vector<int> units((size_t)nparts + 1, nunits);
  for (int p = 0; p < c; ++p) {
    const int64_t w = (int64_t)slots * ((int64_t)gens * p / c);
    units[(size_t)p] = (int)(w < nunits ? w : nunits);
  }
  return units;
}

}  // namespace fs
