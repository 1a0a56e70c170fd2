// fs_format_util.h -- what the format translation units (fs_format.hip, fs_copies.hip) share and nobody else sees:
// timed hipMalloc / hipFree, the scratch pool's handle, and the device idioms of the builders written once -- the two-call
// rocPRIM sorts and scans, the CU count, the one-scalar read-back, the optional copy.
//
// Where a copy's arrays land in HBM and which pool block a scratch request reuses depend on the ORDER of the allocations,
// so the sorts and scans take their temporary storage from a Scratch<char> of the caller: it is allocated inside the call,
// exactly where the written-out form allocated it, and goes back to the pool when the caller's scope ends, as it always did.
#pragma once

#include <chrono>
#include <cstdlib>

#include "fs_common.h"

namespace fs {

// hipMalloc / hipFree with a stopwatch: with FS_TRACE_BUILD set, any single call that takes longer than 50 ms is reported
inline bool trace_build() { static const bool v = getenv("FS_TRACE_BUILD") != nullptr; return v; }

template <typename T>
static hipError_t traced_malloc(T **p, size_t bytes)
{
  if (!trace_build()) return hipMalloc(p, bytes);
  const auto t0 = std::chrono::steady_clock::now();
  const hipError_t e = hipMalloc(p, bytes);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (ms > 50.0) fprintf(stderr, "[fastsparse] hipMalloc of %.1f MB took %.0f ms\n", bytes / 1048576.0, ms);
  return e;
}

inline hipError_t traced_free(void *p)
{
  if (!trace_build()) return hipFree(p);
  const auto t0 = std::chrono::steady_clock::now();
  const hipError_t e = hipFree(p);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (ms > 50.0) fprintf(stderr, "[fastsparse] hipFree took %.0f ms\n", ms);
  return e;
}

// the scratch pool of the format builders (one instance, fs_format.hip)
hipError_t pool_alloc(void **out, size_t bytes);
void pool_free(void *p);

// device scratch that is released (to the pool) on every exit path
template <typename T>
struct Scratch {
  T *p = nullptr;
  size_t bytes = 0;            // what alloc asked for
  Scratch() = default;
  Scratch(const Scratch &) = delete;
  Scratch &operator=(const Scratch &) = delete;
  ~Scratch() { if (p) pool_free(p); }
  hipError_t alloc(size_t n) { bytes = sizeof(T) * (n ? n : 1); return pool_alloc(reinterpret_cast<void **>(&p), bytes); }
  operator T *() const { return p; }
};

// what a handle's copies hold is freed in fs_format.hip (free_csr); the builders free a copy that failed or lost the race
void free_tiled_slot(TiledCsr *&T);
void free_long_rows(LongRows *&L);
void free_binned_slot(BinnedCsr *&N);

constexpr float kLdsxClearWin = 1000.f;    // entries per tile from which the LDS-staged copy is not raced against the others
int two_pass_clear_win(DeviceCsr &A, hipStream_t s, bool *win);   // fs_copies.hip: the two-pass copy, just built, beats the L2-tiled kernel's best

struct BuildClock {
  hipStream_t s;
  std::chrono::steady_clock::time_point t;
  explicit BuildClock(hipStream_t st) : s(st) { (void)hipStreamSynchronize(s); t = std::chrono::steady_clock::now(); }
  float lap()      // ms since the last lap, the stream drained (a handful of synchronisations per matrix built)
  {
    (void)hipStreamSynchronize(s);
    const auto n = std::chrono::steady_clock::now();
    const float ms = std::chrono::duration<float, std::milli>(n - t).count();
    t = n;
    return ms;
  }
};

inline unsigned grid_for(int64_t n) { return (unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1); }

// compute units of the current device, 256 if the query fails
inline int cu_count()
{
  int dev = 0, ncu = 256;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ncu = prop.multiProcessorCount;
  return ncu;
}

// one scalar from the device, the stream drained: the flag / counter a kernel has just set
template <typename T>
static int read_back(T *host, const T *dev, hipStream_t s)
{
  FS_HIP(hipMemcpyAsync(host, dev, sizeof(T), hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  return FS_OK;
}

// An optional copy: if its build failed or did not finish, the slot is freed and the HIP error cleared -- the matrix stays
// usable on the other kernels.
template <typename C, typename F>
static int optional_copy(int rc, C *&slot, F free_fn)
{
  if (rc != FS_OK || (slot && !slot->built)) {
    free_fn(slot);
    (void)hipGetLastError();
  }
  return FS_OK;
}

// bits a radix sort of keys in [0, n) has to look at, at most max_bits (31 for int keys, 32 for unsigned ones)
inline int sort_bits(uint64_t n, int max_bits)
{
  int bits = 1;
  while (bits < max_bits && (1ull << bits) < n) ++bits;
  return bits;
}

// ---- device idioms, defined once in fs_format.hip (rocPRIM and the kernels behind them are compiled there only) ----------
int device_iota(int64_t n, unsigned *idx, hipStream_t s);                                         // idx[i] = i
int device_run_ptr(int64_t nruns, int64_t n, const unsigned *sorted_keys, int *run_ptr, hipStream_t s);   // run_ptr[k] = first position
                                                                                                  // with key >= k, k = 0 .. nruns

// stable radix sort of keys WITH THEIR ENTRY INDICES over the low `bits` bits, separate in / out buffers: idx_in is overwritten
// with 0 .. n - 1 here, idx_out is the permutation
int device_sort_indexed(Scratch<char> &tmp, const int *keys_in, int *keys_out, unsigned *idx_in, unsigned *idx_out, size_t n, int bits,
                      hipStream_t s);
int device_sort_indexed(Scratch<char> &tmp, unsigned char *keys_in, unsigned char *keys_out, unsigned *idx_in, unsigned *idx_out, size_t n,
                      int bits, hipStream_t s);
// stable radix sort of (key, value) pairs AS GIVEN, ping-pong between two key / value buffers the caller already holds: both
// pairs are overwritten (rocprim's plain form would allocate
// a third pair as temporary storage: 4.9 GB at config 3's size, and hipMalloc of such a block was caught taking 4 s);
// *keys / *vals = the buffers that hold the result
int device_sort_pairs(Scratch<char> &tmp, unsigned *k0, unsigned *k1, unsigned *v0, unsigned *v1, size_t n, int bits, hipStream_t s,
                      const unsigned **keys, const unsigned **vals);

// exclusive prefix sums; a tmp that is already allocated is used again (two scans of one size share it) and refused with
// FS_ERR_ARG when it is too small for this scan
int device_exclusive_scan(Scratch<char> &tmp, int *in, int *out, size_t n, hipStream_t s);
int device_exclusive_scan(Scratch<char> &tmp, unsigned *in, unsigned *out, size_t n, hipStream_t s);

}  // namespace fs
