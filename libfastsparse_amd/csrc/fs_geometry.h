// fs_geometry.h -- the geometry constants of the kernels and of their copies, without any HIP type: included by
// fs_common.h (which describes the structures they belong to: TiledCsr, BinnedCsr, LongRows) and by fs_plan.h, whose
// host planners compile with a plain C++ compiler.
#pragma once

namespace fs {

constexpr int kTiledBlock = 1024;      // threads per workgroup of the tiled kernel: ONE workgroup per CU (two
                                       // co-resident workgroups were measured to run at different speeds -- the
                                       // older one wins issue arbitration, 401 vs 450 us per panel -- which pulls
                                       // the band sweep of an XCD apart and out of its L2)
constexpr int kTiledProd = 512;        // waves 0-7 produce (stream + gather), waves 8-15 consume (LDS reduction)
constexpr int kTiledItem = 2048;       // entries per work item (4 per producer thread)
constexpr int kTiledRowsMax = 13056;   // R <= this: 102 KiB of y per workgroup
constexpr int kTiledColBits = 18;      // W <= 262144 columns (2 MiB of x); the other 14 bits are the local row

constexpr int kLdsxRows = 14336;       // LDS-staged kernel: rows per panel (112 KiB of y in LDS, + 3 x 16 KiB slices = 160 KiB)
constexpr int kLdsxCols = 2048;        //                    columns per band: one 16 KiB slice of x, two slices in LDS

constexpr int kBinBlock = 1024;        // threads per workgroup, both passes
constexpr int kBinCols = 16384;        // columns per band: 128 KiB of x in LDS, one pass-1 workgroup per CU
constexpr int kBinRowsMax = 16384;     // rows per panel: 128 KiB of y in LDS, one pass-2 workgroup per CU (measured equal to
                                       // 8192 rows x two workgroups; larger panels mean longer runs, less padding)
// short runs (a power-law shard with a very wide x: config 5, 66 entries per run) pay 7.5 padding entries per run: such
// matrices get bands and panels as large as LDS allows, 19 % fewer bands and panels, 29 % fewer runs (config-5 shard 2.84 ->
// 2.72 ms; config 2, 344 entries per run, was measured 1 % slower with them and keeps the power-of-two sizes)
constexpr int kBinColsBig = 19456, kBinRowsBig = 19456;   // 152 KiB of x / of y in LDS
constexpr int kBinBigRunEntries = 192;                     // chosen below this many entries per run (single-vector copies)
static_assert(kBinColsBig % 1024 == 0 && kBinColsBig < 65536, "band loads are 1024 threads wide; 16-bit local ids");
static_assert(kBinCols % 1024 == 0 && kBinCols % 4 == 0 && kBinRowsMax % 4 == 0 && kBinCols < 65536 && kBinRowsMax <= 65536,
              "band loads are 1024 threads wide; 16-bit local ids; k-column copies divide both by 2 and 4");
#ifndef FS_BIN_GROUP_LOG          // (experiment builds only, FS_HIPCC_EXTRA=-DFS_BIN_GROUP_LOG=5: 256-byte groups, profiles/r05_c2_group32_ab.txt)
#define FS_BIN_GROUP_LOG 4
#endif
constexpr int kBinGroupLog = FS_BIN_GROUP_LOG;
constexpr int kBinGroup = 1 << kBinGroupLog;  // entries per group = one 128-byte L2 line of products (runs that start on half
                                               // lines were measured 19 % slower in pass 1: 0.459 vs 0.386 ms)
constexpr int kBinShareMin = 8192;     // a pass-1 workgroup streams at least this many entries

// two geometries of the 152 KiB of LDS of the long rows' kernel: a wide band with few accumulators, or a narrower band with
// four times as many rows
constexpr int kLongBandA = 16384, kLongRowsA = 3072;      // 128 KiB of x + 24 KiB of accumulators
constexpr int kLongBandB = 8192, kLongRowsB = 12032;      //  64 KiB of x + 94 KiB of accumulators (160 KiB with the zero slots)
constexpr int kLongOwners = kBinBlock / 64;               // the waves of a workgroup: every long row belongs to one of them

}  // namespace fs
