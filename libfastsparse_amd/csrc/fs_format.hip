// fs_format.hip -- one-time format work on the device: the builders' scratch pool and what frees a handle's arrays, chunk
// schedule of the streaming SpMV kernel, index validation, stable COO -> CSR, bucketing, CSR -> CSR of the transpose, the
// partition behind the distributed transpose, synthetic generators.  The re-ordered device copies and the timed choice
// between them are built in fs_copies.hip; the idioms both files share are in fs_format_util.h.
//
// The reference builds its CSRs on the host with a stable counting sort (new_csr csr.h:375-422,
// new_bcsr csr.h:30-67).  Here the same result (entries of a row kept in input order) comes
// from a stable LSD radix sort of (row key, entry index) pairs -- rocPRIM's device radix sort is
// used for this one-time step; the products themselves run on the hand-written kernels of
// fs_kernels.hip.
#include <cstring>
#include <string.h>

#include <algorithm>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "fs_format_util.h"

namespace fs {

// Device scratch of the format builders goes through a small pool: building one matrix takes three candidate copies,
// each with half a dozen temporaries of nnz elements, and hipMalloc of a multi-GB block now and then stalls for SECONDS on
// this platform (FS_TRACE_BUILD: "hipMalloc of 4921.0 MB took 4160 ms"; a copy that usually builds in 71 ms then takes
// 3.4 s).  Blocks freed by one builder are reused by the next, and up to FS_SCRATCH_POOL_MB of idle blocks stay for the
// next creation (pool_trim).
struct PoolBlock { void *p; size_t bytes; bool used; int device; };   // a block serves its own device only (fs_dist_*)
static std::mutex g_pool_lock;
static std::vector<PoolBlock> g_pool;

hipError_t pool_alloc(void **out, size_t bytes)
{
  if (bytes == 0) bytes = 1;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> g(g_pool_lock);
  int best = -1;
  for (int i = 0; i < (int)g_pool.size(); ++i)
    if (!g_pool[i].used && g_pool[i].device == dev && g_pool[i].bytes >= bytes && g_pool[i].bytes <= 4 * bytes + (1 << 20) &&
        (best < 0 || g_pool[i].bytes < g_pool[best].bytes)) best = i;
  if (best >= 0) { g_pool[best].used = true; *out = g_pool[best].p; return hipSuccess; }
  void *p = nullptr;
  hipError_t e = traced_malloc(&p, bytes);
  if (e != hipSuccess) {                      // out of memory: give back what the pool holds idle and try once more
    (void)hipGetLastError();
    for (size_t i = 0; i < g_pool.size();) {
      if (!g_pool[i].used) { (void)traced_free(g_pool[i].p); g_pool.erase(g_pool.begin() + i); } else ++i;
    }
    e = traced_malloc(&p, bytes);
    if (e != hipSuccess) return e;
  }
  g_pool.push_back(PoolBlock{p, bytes, true, dev});
  *out = p;
  return hipSuccess;
}

void pool_free(void *p)
{
  std::lock_guard<std::mutex> g(g_pool_lock);
  for (PoolBlock &b : g_pool)
    if (b.p == p) { b.used = false; return; }
  (void)traced_free(p);
}

// End of a top-level creation: idle blocks are kept for the next one up to FS_SCRATCH_POOL_MB (default 8192; 0 keeps
// nothing), the rest is freed, smallest first -- the big blocks are the ones hipMalloc stalls on.  fs_release_all() empties it.
void pool_trim(bool everything)
{
  static const size_t cap = [] { const char *v = getenv("FS_SCRATCH_POOL_MB"); return (size_t)(v && *v ? atoll(v) : 8192) << 20; }();
  std::lock_guard<std::mutex> g(g_pool_lock);
  for (;;) {
    size_t idle = 0;
    int smallest = -1;
    for (int i = 0; i < (int)g_pool.size(); ++i)
      if (!g_pool[i].used) {
        idle += g_pool[i].bytes;
        if (smallest < 0 || g_pool[i].bytes < g_pool[smallest].bytes) smallest = i;
      }
    if (smallest < 0 || (!everything && idle <= cap)) return;
    (void)traced_free(g_pool[smallest].p);
    g_pool.erase(g_pool.begin() + smallest);
  }
}

void free_tiled_slot(TiledCsr *&T)
{
  if (!T) return;
  void *owned[] = {T->pk, T->vals, T->items, T->item_ptr, T->panel_row, T->vfirst, T->yv, T->chunk_panel, T->chunk_item,
                   T->chunk_ord, T->ticket ? T->ticket - 1 : nullptr};   // (ticket[-1] = the give-up counter: one block)
  for (void *q : owned)
    if (q) (void)traced_free(q);
  delete T;
  T = nullptr;
}

void free_long_rows(LongRows *&L)
{
  if (!L) return;
  void *owned[] = {L->row, L->lcol, L->lrow, L->vals, L->band_ptr, L->seg_ptr, L->ylong, L->ypart};
  for (void *q : owned)
    if (q) (void)traced_free(q);
  delete L;
  L = nullptr;
}

void free_binned_slot(BinnedCsr *&N)
{
  if (!N) return;
  free_long_rows(N->lr);
  void *owned[] = {N->lcol, N->vals, N->gdst, N->lrow, N->lrow8, N->gbase, N->prod, N->band_ptr, N->bin_ptr, N->panel_row, N->vfirst, N->yv};
  for (void *q : owned)
    if (q) (void)traced_free(q);
  delete N;
  N = nullptr;
}

void free_csr(DeviceCsr &A)
{
  if (A.owns) {
    if (A.row_ptr) (void)traced_free(A.row_ptr);
    if (A.cols) (void)traced_free(A.cols);
    if (A.vals) (void)traced_free(A.vals);
  }
  if (A.first_row) (void)traced_free(A.first_row);
  if (A.head) (void)traced_free(A.head);
  if (A.tail) (void)traced_free(A.tail);
  free_tiled_slot(A.tiled);
  free_tiled_slot(A.tiledx);
  free_binned_slot(A.binned);
  free_binned_slot(A.binned2);
  free_binned_slot(A.binned4);
  if (A.spmm_scratch) { (void)traced_free(A.spmm_scratch); A.spmm_scratch = nullptr; A.spmm_scratch_doubles = 0; }
  A = DeviceCsr();
}

int need_plain_csr(const DeviceCsr &A, const char *who)
{
  if (!A.released) return FS_OK;
  set_error(std::string(who) + " reads the plain CSR arrays, which fs_matrix_release_csr gave back (fs_matrix_restore_csr hands them in again)");
  return FS_ERR_RELEASED;
}

// the plain arrays and the chunk schedule of a matrix whose products run on a kept re-ordered copy: owned arrays freed, borrowed ones
// forgotten.  Products in parts keep their cached cuts (they come from the copy's panel tables).
int release_plain_csr(DeviceCsr &A)
{
  const bool kept = (A.binned && A.binned->built) || (A.tiledx && A.tiledx->built) || (A.tiled && A.tiled->built);
  if (A.released || !kept) return 0;
  A.released_valued = A.vals != nullptr;
  if (A.owns) {
    if (A.row_ptr) (void)traced_free(A.row_ptr);
    if (A.cols) (void)traced_free(A.cols);
    if (A.vals) (void)traced_free(A.vals);
  }
  A.row_ptr = nullptr; A.cols = nullptr; A.vals = nullptr;
  for (void **p : {(void **)&A.first_row, (void **)&A.head, (void **)&A.tail})
    if (*p) { (void)traced_free(*p); *p = nullptr; }
  A.released = true;
  return 1;
}

int release_prepared(DeviceCsr &A, int k)
{
  int n = 0;
  if ((k == 0 || k == 2 || k == 3) && A.binned2) { free_binned_slot(A.binned2); A.tried2 = false; ++n; }
  if ((k == 0 || k == 4) && A.binned4) { free_binned_slot(A.binned4); A.tried4 = false; ++n; }
  if (A.spmm_scratch && (k == 0 || (k >= 2 && k <= 16))) {
    // the column-major scratch serves every k up to the largest prepared: it goes when the last k that used it goes (k = 0: now)
    bool others = false;
    if (k != 0) { A.spmm_choice[k] = 0; for (int j = 2; j <= 16; ++j) others = others || (j != k && A.spmm_choice[j] != 0); }
    if (!others) {
      (void)traced_free(A.spmm_scratch); A.spmm_scratch = nullptr; A.spmm_scratch_doubles = 0; ++n;
      for (int j = 0; j <= 16; ++j) A.spmm_choice[j] = 0;
    }
  }
  A.partk[0] = DeviceCsr::PartCuts(); A.partk[1] = DeviceCsr::PartCuts();
  return n;
}

// HBM held by a handle's CSR and every copy / scratch made for it so far, in bytes: [0] the CSR itself (0 when the arrays
// are borrowed) + chunk schedule, [1] the kept single-vector copy (two-pass incl. its product stream, L2-tiled or LDS-staged),
// [2] the k-column two-pass copies (k = 2, 4) and the column-major scratch of multi-column products
void device_bytes(const DeviceCsr &A, int64_t out[3])
{
  auto tiled_bytes = [&](const TiledCsr *T) -> int64_t {
    if (!T) return 0;
    int64_t b = 4 * A.nnz + (T->vals ? 8 * A.nnz : 0) + 16ll * T->nitems + 4ll * (T->P + 1) * 2;
    if (T->vfirst) b += 4ll * (A.nrow + 1);
    if (T->yv) b += 8ll * (T->split ? T->nvrow : A.nrow);
    b += 16ll * T->nchunks + (T->ticket ? 4ll * T->P : 0);
    return b;
  };
  auto binned_bytes = [&](const BinnedCsr *N) -> int64_t {
    if (!N) return 0;
    int64_t b = N->n * (2 + (N->lrow8 ? 1 : 0) + (N->lrow ? 2 : 0) + 8ll * N->kw + (N->vals ? 8 : 0)) + (N->lrow8 ? 6 : 4) * (N->n / (kBinGroup / N->kw)) +
                4ll * (N->B + 1) + 8ll * (N->P + 1);
    if (N->vfirst) b += 4ll * (A.nrow + 1);
    if (N->yv) b += 8ll * N->nvrow * N->kw;
    if (N->lr) b += N->lr->n * (4 + (N->lr->vals ? 8 : 0)) + 12ll * N->lr->nlong + (8ll + 4ll * (kLongOwners + 1)) * (N->lr->B + 1) +
                    8ll * N->lr->nwg * N->lr->nlong;
    return b;
  };
  out[0] = A.released ? 0 : (A.owns ? 4ll * (A.nrow + 1) + 4 * A.nnz + (A.vals ? 8 * A.nnz : 0) : 0) + 4ll * (A.nchunks + 1) + 16ll * A.nchunks;
  out[1] = tiled_bytes(A.tiled) + tiled_bytes(A.tiledx) + binned_bytes(A.binned);
  out[2] = binned_bytes(A.binned2) + binned_bytes(A.binned4) + 8ll * (int64_t)A.spmm_scratch_doubles;
}

// first index r in [0, n] with a[r] >= key (a non-decreasing)
__device__ __forceinline__ int lower_bound_dev(const int *__restrict__ a, int n, int64_t key)
{
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int64_t)a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// first_row[c] = first row whose first non-zero index is >= c*kChunk; first_row[nchunks] = nrow
__global__ void schedule_kernel(int nrow, int nchunks, const int *__restrict__ row_ptr, int *__restrict__ first_row)
{
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > nchunks) return;
  first_row[c] = (c == nchunks) ? nrow : lower_bound_dev(row_ptr, nrow, (int64_t)c * kChunk);
}

__global__ void count_spanning_kernel(int nchunks, int64_t nnz, const int *__restrict__ row_ptr,
                                      const int *__restrict__ first_row, int *__restrict__ count)
{
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nchunks) return;
  const int r0 = first_row[c], r1 = first_row[c + 1];
  if (r1 <= r0) return;
  int64_t e = (int64_t)(c + 1) * kChunk;
  if (e > nnz) e = nnz;
  if ((int64_t)row_ptr[r1] > e) atomicAdd(count, 1);
}


int build_schedule(DeviceCsr &A, hipStream_t s, bool allow_tiled)
{
  BuildClock clock(s);
  A.nchunks = (int)((A.nnz + kChunk - 1) / kChunk);
  if (A.nchunks < 1) A.nchunks = 1;
  FS_HIP(traced_malloc(&A.first_row, sizeof(int) * ((size_t)A.nchunks + 1)));
  FS_HIP(traced_malloc(&A.head, sizeof(double) * (size_t)A.nchunks));
  FS_HIP(traced_malloc(&A.tail, sizeof(double) * (size_t)A.nchunks));
  FS_HIP(hipMemsetAsync(A.head, 0, sizeof(double) * (size_t)A.nchunks, s));
  FS_HIP(hipMemsetAsync(A.tail, 0, sizeof(double) * (size_t)A.nchunks, s));
  const int n = A.nchunks + 1;
  hipLaunchKernelGGL(schedule_kernel, dim3((n + 255) / 256), dim3(256), 0, s, A.nrow, A.nchunks, A.row_ptr,
                     A.first_row);
  FS_HIP(hipGetLastError());
  Scratch<int> cnt;
  FS_HIP(cnt.alloc(1));
  FS_HIP(hipMemsetAsync(cnt, 0, sizeof(int), s));
  hipLaunchKernelGGL(count_spanning_kernel, dim3((A.nchunks + 255) / 256), dim3(256), 0, s, A.nchunks, A.nnz,
                     A.row_ptr, A.first_row, cnt);
  FS_HIP(hipGetLastError());
  if (int rc = read_back(&A.spanning, cnt.p, s)) return rc;
  A.build_ms[2] = clock.lap();
  if (!allow_tiled) return FS_OK;
  // where the one-time format work goes: kept per matrix (fs_matrix_build_ms); FS_TRACE_BUILD=1 also prints it
  // The LDS-staged copy first: where its tiles are dense (config 3: 1 700 entries per tile) it beats the two-pass pair and the
  // L2-tiled kernel two- to threefold (0.68 against 2.2 and 1.9 ms, measured by this builder for four rounds), and building and
  // timing those two only to free them again cost 135 of config 3's 475 ms per matrix and 13 GB of transient HBM.  From
  // kLdsxClearWin entries per tile on they are not built (auto mode; near the crossover -- 500 per tile -- all candidates still race).
  if (int rc = build_tiledx(A, s)) return rc;
  A.build_ms[5] = clock.lap();
  const bool ldsx_clear_win = A.tiledx && A.tiledx->built && A.tiledx->entries_per_tile >= kLdsxClearWin && options().binning != 2 &&
                              options().tiling != 2 && (A.tiledx->orderable || !options().reproducible);   // (a copy that cannot give the
                                                                              // fixed-order sums asked for needs its rivals)
  if (!ldsx_clear_win)
    if (int rc = build_binned(A, s)) return rc;
  bool binned_clear_win = false;
  if (!ldsx_clear_win)
    if (int rc = two_pass_clear_win(A, s, &binned_clear_win)) return rc;
  A.two_pass_clear_win = binned_clear_win;
  A.build_ms[3] = clock.lap();
  if (!ldsx_clear_win && !binned_clear_win)
    if (int rc = build_tiled(A, s)) return rc;
  A.build_ms[4] = clock.lap();
  const int rc = choose_copy(A, s);        // fills build_ms[6] (timing) and starts [7] (freeing the losers)
  pool_trim();
  A.build_ms[7] += clock.lap() - A.build_ms[6];
  if (trace_build())
    fprintf(stderr, "[fastsparse] %d x %d, %lld nnz: schedule %.1f ms, two-pass copy %.1f ms, tiled copy %.1f ms, LDS-staged copy %.1f ms, "
            "candidates timed %.1f ms, losers freed %.1f ms\n", A.nrow, A.ncol, (long long)A.nnz, A.build_ms[2], A.build_ms[3], A.build_ms[4],
            A.build_ms[5], A.build_ms[6], A.build_ms[7]);
  return rc;
}

// ---- stable COO -> CSR -----------------------------------------------------------------------
__global__ void iota_kernel(int64_t n, unsigned *__restrict__ idx)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) idx[i] = (unsigned)i;
}

int device_iota(int64_t n, unsigned *idx, hipStream_t s)
{
  hipLaunchKernelGGL(iota_kernel, dim3(grid_for(n)), dim3(256), 0, s, n, idx);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// The two-call rocPRIM pattern, once per primitive: size query, temporary storage from the caller's Scratch, the real call.
template <typename KeysIn, typename K>
static int sort_indexed(Scratch<char> &tmp, KeysIn keys_in, K *keys_out, unsigned *idx_in, unsigned *idx_out, size_t n, int bits, hipStream_t s)
{
  if (int rc = device_iota((int64_t)n, idx_in, s)) return rc;
  size_t tmp_bytes = 0;
  FS_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys_in, keys_out, idx_in, idx_out, n, 0, bits, s));
  FS_HIP(tmp.alloc(tmp_bytes));
  FS_HIP(rocprim::radix_sort_pairs((void *)tmp.p, tmp_bytes, keys_in, keys_out, idx_in, idx_out, n, 0, bits, s));
  return FS_OK;
}

int device_sort_indexed(Scratch<char> &tmp, const int *keys_in, int *keys_out, unsigned *idx_in, unsigned *idx_out, size_t n, int bits,
                      hipStream_t s)
{
  return sort_indexed(tmp, keys_in, keys_out, idx_in, idx_out, n, bits, s);
}

int device_sort_indexed(Scratch<char> &tmp, unsigned char *keys_in, unsigned char *keys_out, unsigned *idx_in, unsigned *idx_out, size_t n,
                      int bits, hipStream_t s)
{
  return sort_indexed(tmp, keys_in, keys_out, idx_in, idx_out, n, bits, s);
}

int device_sort_pairs(Scratch<char> &tmp, unsigned *k0, unsigned *k1, unsigned *v0, unsigned *v1, size_t n, int bits, hipStream_t s,
                      const unsigned **keys, const unsigned **vals)
{
  rocprim::double_buffer<unsigned> dk(k0, k1), dv(v0, v1);
  size_t tmp_bytes = 0;
  FS_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, dk, dv, n, 0, bits, s));     // stable: input order inside a run
  FS_HIP(tmp.alloc(tmp_bytes));
  FS_HIP(rocprim::radix_sort_pairs((void *)tmp.p, tmp_bytes, dk, dv, n, 0, bits, s));
  *keys = dk.current();
  *vals = dv.current();
  return FS_OK;
}

template <typename T>
static int exclusive_scan(Scratch<char> &tmp, T *in, T *out, size_t n, hipStream_t s)
{
  size_t tmp_bytes = 0;
  FS_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, in, out, (T)0, n, rocprim::plus<T>(), s));
  if (!tmp.p) FS_HIP(tmp.alloc(tmp_bytes));
  if (tmp.bytes < tmp_bytes) { set_error("exclusive_scan: the shared temporary is too small for this scan"); return FS_ERR_ARG; }
  FS_HIP(rocprim::exclusive_scan((void *)tmp.p, tmp_bytes, in, out, (T)0, n, rocprim::plus<T>(), s));
  return FS_OK;
}

int device_exclusive_scan(Scratch<char> &tmp, int *in, int *out, size_t n, hipStream_t s) { return exclusive_scan(tmp, in, out, n, s); }
int device_exclusive_scan(Scratch<char> &tmp, unsigned *in, unsigned *out, size_t n, hipStream_t s) { return exclusive_scan(tmp, in, out, n, s); }

__global__ void permute_kernel(int64_t n, const unsigned *__restrict__ perm, const int *__restrict__ cols_in,
                               const double *__restrict__ vals_in, int *__restrict__ cols_out,
                               double *__restrict__ vals_out)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned src = perm[i];
  cols_out[i] = cols_in[src];
  if (vals_in) vals_out[i] = vals_in[src];
}

// row_ptr[r] = first position in the sorted key array whose key is >= r
__global__ void row_ptr_kernel(int nrow, int64_t nnz, const int *__restrict__ sorted_rows, int *__restrict__ row_ptr)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > nrow) return;
  int64_t lo = 0, hi = nnz;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (sorted_rows[mid] < r) lo = mid + 1; else hi = mid;
  }
  row_ptr[r] = (int)lo;
}

static int device_row_ptr(int nrow, int64_t nnz, const int *sorted_rows, int *row_ptr, hipStream_t s)
{
  hipLaunchKernelGGL(row_ptr_kernel, dim3(grid_for((int64_t)nrow + 1)), dim3(256), 0, s, nrow, nnz, sorted_rows, row_ptr);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// ---- index validation at upload -------------------------------------------------------------------------
// The reference validates nothing and a bad index there is a host segfault.  Here it would be a GPU
// memory fault, which can take more than this process down, so every matrix is checked once when it is created:
// columns in [0, ncol), COO rows in [0, nrow), row_ptr starting at 0, ending at nnz and never decreasing.
__global__ void validate_kernel(int64_t nnz, int ncol, int nrow, const int *__restrict__ cols, const int *__restrict__ rows,
                                const int *__restrict__ row_ptr, int *__restrict__ bad)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool b = false;
  if (i < nnz) {
    b = (unsigned)cols[i] >= (unsigned)ncol;
    if (rows) b = b || (unsigned)rows[i] >= (unsigned)nrow;
  }
  if (row_ptr && i <= nrow) {
    const int v = row_ptr[i];
    if (i == 0 && v != 0) b = true;
    if (i == nrow && (int64_t)v != nnz) b = true;
    if (i < nrow && row_ptr[i + 1] < v) b = true;
  }
  if (b) *bad = 1;
}

int validate_indices(int nrow, int ncol, int64_t nnz, const int *row_ptr_dev, const int *rows_dev, const int *cols_dev,
                     hipStream_t s)
{
  Scratch<int> bad;
  FS_HIP(bad.alloc(1));
  FS_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
  const int64_t n = nnz > (int64_t)nrow + 1 ? nnz : (int64_t)nrow + 1;
  hipLaunchKernelGGL(validate_kernel, dim3(grid_for(n)), dim3(256), 0, s, nnz, ncol, nrow, cols_dev, rows_dev, row_ptr_dev, bad.p);
  FS_HIP(hipGetLastError());
  int h = 0;
  if (int rc = read_back(&h, bad.p, s)) return rc;
  if (h) {
    set_error("matrix arrays are inconsistent: a column or row index is out of range, or row_ptr does not run from 0 to nnz "
              "without decreasing");
    return FS_ERR_ARG;
  }
  return FS_OK;
}

int coo_to_csr_device(DeviceCsr &out, int nrow, int ncol, int64_t nnz, const int *rows_dev, const int *cols_dev,
                      const double *vals_dev, hipStream_t s)
{
  BuildClock clock(s);
  out = DeviceCsr();
  out.nrow = nrow; out.ncol = ncol; out.nnz = nnz; out.owns = true;
  const size_t n = (size_t)(nnz > 0 ? nnz : 1);
  FS_HIP(traced_malloc(&out.row_ptr, sizeof(int) * ((size_t)nrow + 1)));
  FS_HIP(traced_malloc(&out.cols, sizeof(int) * n));
  if (vals_dev) FS_HIP(traced_malloc(&out.vals, sizeof(double) * n));
  Scratch<int> keys_out;
  Scratch<unsigned> idx_in, idx_out;
  Scratch<char> tmp;
  FS_HIP(keys_out.alloc(n));
  FS_HIP(idx_in.alloc(n));
  FS_HIP(idx_out.alloc(n));
  if (nnz > 0) {
    if (int rc = device_sort_indexed(tmp, rows_dev, keys_out.p, idx_in.p, idx_out.p, (size_t)nnz, sort_bits((uint64_t)nrow, 31), s)) return rc;
    hipLaunchKernelGGL(permute_kernel, dim3(grid_for(nnz)), dim3(256), 0, s, nnz, idx_out.p, cols_dev, vals_dev,
                       out.cols, out.vals);
    FS_HIP(hipGetLastError());
  }
  if (int rc = device_row_ptr(nrow, nnz, keys_out.p, out.row_ptr, s)) return rc;
  FS_HIP(hipStreamSynchronize(s));
  const float order_ms = clock.lap();
  const int rc = build_schedule(out, s);   // the temporaries above go back to the pool when this function returns; the next
                                           // creation's pool_trim (or fs_release_all) frees them
  out.build_ms[1] += order_ms;
  return rc;
}

// ---- the reference's format constructors on the device ----------------------------------------------------
// new_csr / new_bcsr (csr.h:375-422, 30-67), new_cbcsr (cbcsr.h:16-65) and new_bsbm / new_bsdm (sparse.h:175-213,
// dsparse.h:132-173) are all one operation: a STABLE bucketing of the COO entries by a key -- the row, the
// (column block, row) cell, the row block -- followed by a copy of the payload arrays in bucket order.  On the host
// that is a serial counting sort over nnz entries (seconds at config 3's 640 M); here the arrays are uploaded once,
// ordered by a stable LSD radix sort of (key, entry index), gathered and downloaded.  Same arrays as the host
// builders, element for element (tests/test_gpu_parity.py::test_device_constructors_match_oracle).
__global__ void bucket_key_kernel(int64_t nnz, int kind, int param, int nrow, const int *__restrict__ rows,
                                  const int *__restrict__ cols, int *__restrict__ keys)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  keys[i] = kind == 1 ? (cols[i] / param) * nrow + rows[i] : rows[i] / param;
}

__global__ void bucket_gather_kernel(int64_t nnz, const unsigned *__restrict__ perm, const int *__restrict__ rows,
                                     const int *__restrict__ cols, const double *__restrict__ vals, int *__restrict__ rows_out,
                                     int *__restrict__ cols_out, double *__restrict__ vals_out)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  const unsigned src = perm[i];
  if (rows_out) rows_out[i] = rows[src];
  cols_out[i] = cols[src];
  if (vals_out) vals_out[i] = vals[src];
}

static int bucket_coo_impl(int kind, int param, int nrow, int ncol, int64_t nbuckets, int64_t nnz, const int *rows,
                           const int *cols, const double *vals, int *offsets, int *rows_out, int *cols_out, double *vals_out)
{
  hipStream_t s = nullptr;
  const size_t n = (size_t)(nnz > 0 ? nnz : 1);
  Scratch<int> d_rows, d_cols, d_keys, d_skeys, d_off, d_rows_o, d_cols_o;
  Scratch<double> d_vals, d_vals_o;
  Scratch<unsigned> idx_in, idx_out;
  Scratch<char> tmp;
  FS_HIP(d_rows.alloc(n));
  FS_HIP(d_cols.alloc(n));
  FS_HIP(hipMemcpy(d_rows.p, rows, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice));
  FS_HIP(hipMemcpy(d_cols.p, cols, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice));
  if (int rc = validate_indices(nrow, ncol, nnz, nullptr, d_rows.p, d_cols.p, s)) return rc;
  const int *keys = d_rows.p;
  if (kind != 0) {
    FS_HIP(d_keys.alloc(n));
    hipLaunchKernelGGL(bucket_key_kernel, dim3(grid_for(nnz)), dim3(256), 0, s, nnz, kind, param, nrow, d_rows.p, d_cols.p, d_keys.p);
    FS_HIP(hipGetLastError());
    keys = d_keys.p;
  }
  FS_HIP(d_skeys.alloc(n));
  FS_HIP(idx_in.alloc(n));
  FS_HIP(idx_out.alloc(n));
  FS_HIP(d_off.alloc((size_t)nbuckets + 1));
  if (nnz > 0) {
    if (int rc = device_sort_indexed(tmp, keys, d_skeys.p, idx_in.p, idx_out.p, (size_t)nnz, sort_bits((uint64_t)nbuckets, 31), s)) return rc;
  }
  if (int rc = device_row_ptr((int)nbuckets, nnz, d_skeys.p, d_off.p, s)) return rc;
  FS_HIP(d_cols_o.alloc(n));
  if (rows_out) FS_HIP(d_rows_o.alloc(n));
  if (vals) {
    FS_HIP(d_vals.alloc(n));
    FS_HIP(d_vals_o.alloc(n));
    FS_HIP(hipMemcpy(d_vals.p, vals, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice));
  }
  if (nnz > 0) {
    hipLaunchKernelGGL(bucket_gather_kernel, dim3(grid_for(nnz)), dim3(256), 0, s, nnz, idx_out.p, d_rows.p, d_cols.p,
                       vals ? d_vals.p : nullptr, rows_out ? d_rows_o.p : nullptr, d_cols_o.p, vals ? d_vals_o.p : nullptr);
    FS_HIP(hipGetLastError());
  }
  FS_HIP(hipMemcpy(offsets, d_off.p, sizeof(int) * ((size_t)nbuckets + 1), hipMemcpyDeviceToHost));
  if (nnz > 0) {
    FS_HIP(hipMemcpy(cols_out, d_cols_o.p, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToHost));
    if (rows_out) FS_HIP(hipMemcpy(rows_out, d_rows_o.p, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToHost));
    if (vals) FS_HIP(hipMemcpy(vals_out, d_vals_o.p, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost));
  }
  return FS_OK;
}

// ---- CSR -> CSR of the transpose -------------------------------------------------------------------
// row id of every stored entry (one thread per entry, binary search in row_ptr)
__global__ void expand_rows_kernel(int nrow, int64_t nnz, const int *__restrict__ row_ptr, int *__restrict__ rows)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  int lo = 0, hi = nrow;  // last r with row_ptr[r] <= i
  while (lo < hi) {
    const int mid = lo + ((hi - lo + 1) >> 1);
    if ((int64_t)row_ptr[mid] <= i) lo = mid; else hi = mid - 1;
  }
  rows[i] = lo;
}

// ---- column-blocked binary CSR -> plain pattern-only CSR --------------------------------------------------------
// cell = block * nrow + row, cells stored block-major: a stable sort of the entries by row leaves every row's entries
// block by block and, inside a cell, in storage order -- the order in which the reference's one-thread loop adds them
// (cbcsr.h:88-97).  The plain CSR then goes through the ordinary format builder (copies, timed choice).
__global__ void cell_rows_kernel(int ncell, int nrow, int64_t nnz, const int *__restrict__ cell_ptr, int *__restrict__ rows)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  int lo = 0, hi = ncell;  // last cell with cell_ptr[cell] <= i
  while (lo < hi) {
    const int mid = lo + ((hi - lo + 1) >> 1);
    if ((int64_t)cell_ptr[mid] <= i) lo = mid; else hi = mid - 1;
  }
  rows[i] = lo % nrow;
}

int cbcsr_rows_device(DeviceCsr &out, int nrow, int ncol, int nblocks, int64_t nnz, const int *cell_ptr_dev,
                      const int *cols_dev, hipStream_t s)
{
  Scratch<int> rows;
  FS_HIP(rows.alloc((size_t)nnz));
  hipLaunchKernelGGL(cell_rows_kernel, dim3(grid_for(nnz)), dim3(256), 0, s, nblocks * nrow, nrow, nnz, cell_ptr_dev, rows.p);
  FS_HIP(hipGetLastError());
  return coo_to_csr_device(out, nrow, ncol, nnz, rows.p, cols_dev, nullptr, s);
}

int transpose_device(const DeviceCsr &A, DeviceCsr &At, hipStream_t s)
{
  if (int rc = need_plain_csr(A, "fs_matrix_build_transpose")) return rc;
  BuildClock clock(s);
  Scratch<int> rows;
  const size_t n = (size_t)(A.nnz > 0 ? A.nnz : 1);
  FS_HIP(rows.alloc(n));
  if (A.nnz > 0) {
    hipLaunchKernelGGL(expand_rows_kernel, dim3(grid_for(A.nnz)), dim3(256), 0, s, A.nrow, A.nnz, A.row_ptr, rows.p);
    FS_HIP(hipGetLastError());
  }
  // A' in COO is (cols, rows, vals); stable sort by column keeps the row order inside each column,
  // i.e. the order in which the serial loops of At_mul_B (sparse.h:72-74) visit a column's entries
  // when the COO itself is row ordered.
  const float expand_ms = clock.lap();
  const int rc = coo_to_csr_device(At, A.ncol, A.nrow, A.nnz, A.cols, rows.p, A.vals, s);
  At.build_ms[1] += expand_ms;
  return rc;
}

// ---- row shards of A' from the row shards of A, without any whole-matrix host array -----------------------------------
// (fs_dist_matrix_build_transpose_device, fs_dist.hip).  BASELINE config 5 (3.2 G entries) only exists as per-device shards:
// the rows of A' (= columns of A) are cut by non-zeros from per-shard column counts added up on one device, every shard
// partitions its entries stably by the device that will own their column, the parts travel device to device, and each
// device orders what it received by row of A' with the stable COO -> CSR above.  Sources hold ascending row ranges of A
// and are concatenated in rank order, so every row of A' keeps ascending A-row order: the order a stable column sort of
// the whole matrix gives (what the serial At_mul_B loop, sparse.h:68-75, visits), as fs_matrix_build_transpose on one GPU.
__global__ void column_count_kernel(int64_t nnz, const int *__restrict__ cols, int *__restrict__ counts)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nnz) atomicAdd(&counts[cols[i]], 1);
}

__global__ void add_counts_kernel(int64_t n, int *__restrict__ acc, const int *__restrict__ add)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) acc[i] += add[i];
}

int shard_column_counts(const DeviceCsr &A, int *counts_dev, hipStream_t s)
{
  if (A.nnz <= 0) return FS_OK;
  hipLaunchKernelGGL(column_count_kernel, dim3(grid_for(A.nnz)), dim3(256), 0, s, A.nnz, A.cols, counts_dev);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

int add_counts(int64_t n, int *acc_dev, const int *add_dev, hipStream_t s)
{
  if (n <= 0) return FS_OK;
  hipLaunchKernelGGL(add_counts_kernel, dim3(grid_for(n)), dim3(256), 0, s, n, acc_dev, add_dev);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// bounds[r] = first item b whose exclusive prefix of counts is >= total * r / nparts (nnz_cut of fs_dist.hip on the device)
__global__ void cut_kernel(int n_items, const int64_t *__restrict__ inc, int nparts, int *__restrict__ bounds)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > nparts) return;
  const int64_t total = n_items > 0 ? inc[n_items - 1] : 0;
  if (r == 0) { bounds[0] = 0; return; }
  if (r == nparts) { bounds[nparts] = n_items; return; }
  const int64_t target = total / nparts * r + total % nparts * r / nparts;   // total * r / nparts without overflow
  int lo = 0, hi = n_items;                       // first b in [0, n_items] with prefix(b) >= target, prefix(b) = b ? inc[b - 1] : 0
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int64_t pm = mid ? inc[mid - 1] : 0;
    if (pm < target) lo = mid + 1; else hi = mid;
  }
  bounds[r] = lo;
}

struct IntToI64 { __device__ int64_t operator()(int v) const { return (int64_t)v; } };

// inclusive prefix sums of int counts in 64 bits, in the manner of exclusive_scan above
static int device_inclusive_scan(Scratch<char> &tmp, const int *in, int64_t *out, size_t n, hipStream_t s)
{
  size_t tmp_bytes = 0;
  auto it = rocprim::make_transform_iterator(in, IntToI64());
  FS_HIP(rocprim::inclusive_scan(nullptr, tmp_bytes, it, out, n, rocprim::plus<int64_t>(), s));
  FS_HIP(tmp.alloc(tmp_bytes));
  FS_HIP(rocprim::inclusive_scan((void *)tmp.p, tmp_bytes, it, out, n, rocprim::plus<int64_t>(), s));
  return FS_OK;
}

int cut_by_counts(int n_items, const int *counts_dev, int nparts, int *bounds_host, int64_t *total, hipStream_t s)
{
  Scratch<int64_t> inc;
  Scratch<int> bd;
  Scratch<char> tmp;
  FS_HIP(inc.alloc((size_t)n_items + 1));
  FS_HIP(bd.alloc((size_t)nparts + 1));
  if (n_items > 0)
    if (int rc = device_inclusive_scan(tmp, counts_dev, inc.p, (size_t)n_items, s)) return rc;
  hipLaunchKernelGGL(cut_kernel, dim3(grid_for((int64_t)nparts + 1)), dim3(256), 0, s, n_items, inc.p, nparts, bd.p);
  FS_HIP(hipGetLastError());
  FS_HIP(hipMemcpyAsync(bounds_host, bd.p, sizeof(int) * ((size_t)nparts + 1), hipMemcpyDeviceToHost, s));
  int64_t tot = 0;
  if (n_items > 0) FS_HIP(hipMemcpyAsync(&tot, inc.p + (n_items - 1), sizeof(int64_t), hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  for (int r = 1; r <= nparts; ++r)               // monotone, like nnz_cut
    if (bounds_host[r] < bounds_host[r - 1]) bounds_host[r] = bounds_host[r - 1];
  if (total) *total = tot;
  return FS_OK;
}

constexpr int kMaxParts = 64;

// key = the part that owns column cols[i]: the last d with bounds[d] <= column (empty parts own nothing); counts per part
__global__ __launch_bounds__(256) void dest_key_kernel(int64_t nnz, int nparts, const int *__restrict__ bounds, const int *__restrict__ cols,
                                                      unsigned char *__restrict__ key, unsigned long long *__restrict__ count)
{
  __shared__ int sb[kMaxParts + 1];
  __shared__ unsigned sc[kMaxParts];
  if (threadIdx.x <= nparts) sb[threadIdx.x] = bounds[threadIdx.x];
  if (threadIdx.x < nparts) sc[threadIdx.x] = 0u;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nnz) {
    const int c = cols[i];
    int d = 0;
    for (int r = 1; r < nparts; ++r) d = sb[r] <= c ? r : d;
    key[i] = (unsigned char)d;
    atomicAdd(&sc[d], 1u);
  }
  __syncthreads();
  if (threadIdx.x < nparts && sc[threadIdx.x]) atomicAdd(&count[threadIdx.x], (unsigned long long)sc[threadIdx.x]);
}

__global__ void transpose_gather_kernel(int64_t nnz, int row_lo, const int *__restrict__ bounds, const unsigned char *__restrict__ skey,
                                        const unsigned *__restrict__ perm, const int *__restrict__ rows, const int *__restrict__ cols,
                                        const double *__restrict__ vals, int *__restrict__ trow, int *__restrict__ tcol,
                                        double *__restrict__ tval)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  const unsigned src = perm[i];
  trow[i] = cols[src] - bounds[skey[i]];          // row of A', local to the part that owns it
  tcol[i] = row_lo + rows[src];                   // column of A' = global row of A
  if (vals) tval[i] = vals[src];
}

// The entries of one row shard of A (first global row row_lo) as entries of A', stably partitioned by owning part:
// *trow / *tcol / *tval (hipMalloc'ed here, nnz long; *tval = nullptr for a pattern-only shard) hold part 0's entries first, then
// part 1's ..., each part in the shard's CSR order; count_host[d] = entries of part d.
int shard_transpose_partition(const DeviceCsr &A, int row_lo, int nparts, const int *bounds_host, int **trow, int **tcol,
                              double **tval, int64_t *count_host, hipStream_t s)
{
  *trow = nullptr; *tcol = nullptr; *tval = nullptr;
  for (int d = 0; d < nparts; ++d) count_host[d] = 0;
  if (nparts < 1 || nparts > kMaxParts) { set_error("shard_transpose_partition: 1 to 64 parts"); return FS_ERR_ARG; }
  const size_t n = (size_t)(A.nnz > 0 ? A.nnz : 1);
  FS_HIP(traced_malloc(trow, sizeof(int) * n));
  FS_HIP(traced_malloc(tcol, sizeof(int) * n));
  if (A.vals) FS_HIP(traced_malloc(tval, sizeof(double) * n));
  if (A.nnz <= 0) return FS_OK;
  Scratch<int> rows, bd;
  Scratch<unsigned char> key, skey;
  Scratch<unsigned> idx_in, idx_out;
  Scratch<unsigned long long> cnt;
  Scratch<char> tmp;
  FS_HIP(rows.alloc(n));
  FS_HIP(bd.alloc((size_t)nparts + 1));
  FS_HIP(key.alloc(n));
  FS_HIP(skey.alloc(n));
  FS_HIP(idx_in.alloc(n));
  FS_HIP(idx_out.alloc(n));
  FS_HIP(cnt.alloc((size_t)nparts));
  FS_HIP(hipMemcpyAsync(bd.p, bounds_host, sizeof(int) * ((size_t)nparts + 1), hipMemcpyHostToDevice, s));
  FS_HIP(hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long) * (size_t)nparts, s));
  hipLaunchKernelGGL(expand_rows_kernel, dim3(grid_for(A.nnz)), dim3(256), 0, s, A.nrow, A.nnz, A.row_ptr, rows.p);
  hipLaunchKernelGGL(dest_key_kernel, dim3(grid_for(A.nnz)), dim3(256), 0, s, A.nnz, nparts, bd.p, A.cols, key.p, cnt.p);
  if (int rc = device_sort_indexed(tmp, key.p, skey.p, idx_in.p, idx_out.p, (size_t)A.nnz, sort_bits((uint64_t)nparts, 31), s)) return rc;
  hipLaunchKernelGGL(transpose_gather_kernel, dim3(grid_for(A.nnz)), dim3(256), 0, s, A.nnz, row_lo, bd.p, skey.p, idx_out.p, rows.p,
                     A.cols, A.vals, *trow, *tcol, *tval);
  FS_HIP(hipGetLastError());
  unsigned long long hc[kMaxParts];
  FS_HIP(hipMemcpyAsync(hc, cnt.p, sizeof(unsigned long long) * (size_t)nparts, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  for (int d = 0; d < nparts; ++d) count_host[d] = (int64_t)hc[d];
  return FS_OK;
}

// ---- run pointers of the copies' sorted keys (fs_copies.hip, through device_run_ptr) -------------------------------------
// tile_ptr[k] = first sorted position whose key is >= k, k = 0 .. ntiles
__global__ void tile_ptr_kernel(int64_t ntiles, int64_t nnz, const unsigned *__restrict__ skeys, int *__restrict__ tile_ptr)
{
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > ntiles) return;
  int64_t lo = 0, hi = nnz;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)skeys[mid] < k) lo = mid + 1; else hi = mid;
  }
  tile_ptr[k] = (int)lo;
}

int device_run_ptr(int64_t nruns, int64_t n, const unsigned *sorted_keys, int *run_ptr, hipStream_t s)
{
  hipLaunchKernelGGL(tile_ptr_kernel, dim3(grid_for(nruns + 1)), dim3(256), 0, s, nruns, n, sorted_keys, run_ptr);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// ---- synthetic inputs (same arithmetic as oracle/fs_synth.c) -------------------------------------
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t z)
{
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ void synth_entry(uint64_t seed, int64_t grow, int slot, int ncol, int *c, double *v)
{
  const uint64_t h = splitmix64(seed ^ ((uint64_t)grow * 0x100000001B3ull + (uint64_t)slot));
  *c = (int)__umul64hi(h, (uint64_t)ncol);
  const uint64_t h2 = splitmix64(h ^ 0xABCDEF0123456789ull);
  *v = (double)(h2 >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

__global__ void synth_uniform_kernel(int nrow, int ncol, int per_row, uint64_t seed, int64_t row_offset,
                                     int *__restrict__ row_ptr, int *__restrict__ cols, double *__restrict__ vals)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nnz = (int64_t)nrow * per_row;
  if (i <= nrow && row_ptr) row_ptr[i] = (int)(i * per_row);
  if (i >= nnz) return;
  const int64_t r = i / per_row;
  const int slot = (int)(i - r * per_row);
  int c; double v;
  synth_entry(seed, row_offset + r, slot, ncol, &c, &v);
  cols[i] = c;
  if (vals) vals[i] = v;
}

__global__ void synth_lengths_kernel(int nrow, double scale, int max_len, uint64_t seed, int64_t row_offset,
                                     int *__restrict__ len)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrow) return;
  const uint64_t h = splitmix64(seed ^ (0xC0FFEEull + (uint64_t)(row_offset + r) * 0x9E3779B97F4A7C15ull));
  const double u = (double)((h >> 11) + 1) * (1.0 / 9007199254740992.0);  // (0, 1]
  double L = scale / u;
  if (L > (double)max_len) L = (double)max_len;
  int n = (int)L;
  len[r] = n < 1 ? 1 : n;
}

__global__ void synth_fill_kernel(int nrow, int ncol, uint64_t seed, int64_t row_offset,
                                  const int *__restrict__ row_ptr, int *__restrict__ cols, double *__restrict__ vals)
{
  // one wave per row, lanes stride over the row's slots
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (w >= nrow) return;
  const int a = row_ptr[w], b = row_ptr[w + 1];
  for (int64_t i = (int64_t)a + lane; i < b; i += 64) {
    int c; double v;
    synth_entry(seed, row_offset + w, (int)(i - a), ncol, &c, &v);
    cols[i] = c;
    if (vals) vals[i] = v;
  }
}

}  // namespace fs

extern "C" {

int fs_bucket_coo(int kind, int param, int nrow, int ncol, int64_t nbuckets, int64_t nnz, const int *rows, const int *cols,
                  const double *vals, int *offsets, int *rows_out, int *cols_out, double *vals_out)
{
  if (kind < 0 || kind > 2 || (kind != 0 && param < 1) || nrow < 0 || nbuckets < 0 || nbuckets >= (1ll << 31) || nnz < 0 ||
      nnz >= (1ll << 31) || !offsets || (nnz > 0 && (!rows || !cols || !cols_out)) || (vals && !vals_out)) {
    fs::set_error("fs_bucket_coo: bad argument");
    return FS_ERR_ARG;
  }
  const int rc = fs::bucket_coo_impl(kind, param, nrow, ncol, nbuckets, nnz, rows, cols, vals, offsets, rows_out, cols_out, vals_out);
  fs::pool_trim();
  return rc;
}

/* should a constructor given nnz entries build on the device?  option device_build: 0 never, 1 when a device is
 * visible and the matrix has at least 4 M entries (below that the host loop is faster than the PCIe round trip),
 * 2 whenever a device is visible; the environment variable FS_DEVICE_BUILD sets the option's initial value */
int fs_device_build_wanted(int64_t nnz)
{
  static const int env = [] { const char *v = getenv("FS_DEVICE_BUILD"); return v && *v ? atoi(v) : -1; }();
  int mode = fs::options().device_build;
  if (mode < 0) mode = env >= 0 ? env : 1;
  if (mode == 0) return 0;
  static const int ndev = [] { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; } return n; }();
  if (ndev < 1) return 0;
  return mode == 2 || nnz >= (4 << 20);
}

int fs_synth_uniform(int nrow, int ncol, int per_row, uint64_t seed, int64_t row_offset, int *row_ptr_dev,
                     int *cols_dev, double *vals_dev, fs_stream_t stream)
{
  if (nrow < 0 || ncol < 1 || per_row < 0 || !cols_dev) { fs::set_error("fs_synth_uniform: bad argument"); return FS_ERR_ARG; }
  int64_t n = (int64_t)nrow * per_row;
  if (n < (int64_t)nrow + 1) n = (int64_t)nrow + 1;
  hipLaunchKernelGGL(fs::synth_uniform_kernel, dim3(fs::grid_for(n)), dim3(256), 0, (hipStream_t)stream, nrow, ncol,
                     per_row, seed, row_offset, row_ptr_dev, cols_dev, vals_dev);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

int fs_synth_powerlaw_lengths(int nrow, double scale, int max_len, uint64_t seed, int64_t row_offset, int *len_dev,
                              fs_stream_t stream)
{
  if (nrow < 0 || !len_dev || max_len < 1) { fs::set_error("fs_synth_powerlaw_lengths: bad argument"); return FS_ERR_ARG; }
  hipLaunchKernelGGL(fs::synth_lengths_kernel, dim3(fs::grid_for(nrow)), dim3(256), 0, (hipStream_t)stream, nrow,
                     scale, max_len, seed, row_offset, len_dev);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

int fs_synth_fill(int nrow, int ncol, uint64_t seed, int64_t row_offset, const int *row_ptr_dev, int *cols_dev,
                  double *vals_dev, fs_stream_t stream)
{
  if (nrow < 0 || ncol < 1 || !row_ptr_dev || !cols_dev) { fs::set_error("fs_synth_fill: bad argument"); return FS_ERR_ARG; }
  hipLaunchKernelGGL(fs::synth_fill_kernel, dim3(fs::grid_for((int64_t)nrow * 64)), dim3(256), 0, (hipStream_t)stream,
                     nrow, ncol, seed, row_offset, row_ptr_dev, cols_dev, vals_dev);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

}  // extern "C"
