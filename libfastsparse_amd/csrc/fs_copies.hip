// fs_copies.hip -- the re-ordered device copies of a CSR and the timed choice between them: virtual rows (long rows cut into
// pieces), the L2-tiled copy and its LDS-staged form (with ldsx_reorder_kernel, which arranges every work item for the LDS
// banks), the two-pass copy, the long rows taken out of it, and choose_copy, which times the candidates and keeps the fastest.
//
// A builder reads: reject, virtual rows, plan, allocate, sort, pack, upload.  The plans -- every decision taken on the host --
// are the plain functions of fs_plan.h; the device idioms (sorts, scans, scalar read-back) are in fs_format_util.h.  The ORDER
// of the allocations here is part of the behaviour: it decides where a copy's arrays land in HBM.
#include <algorithm>
#include <vector>

#include "fs_format_util.h"
#include "fs_plan.h"

namespace fs {

static_assert(sizeof(WorkItem) == sizeof(int4) && sizeof(RowLen) == sizeof(int2), "fs_plan.h's plain structs are the device's int4 / int2");

// ---- L2-tiled copy ---------------------------------------------------------------------------------
// Long rows are cut into pieces of at most `split` consecutive entries ("virtual rows"): the tiled kernel then
// never meets a row that dwarfs a panel or a run that one lane has to walk for long, and the pieces' sums are
// added per row, in storage order, by a combine pass.  A matrix without long rows is its own virtual matrix.
__global__ void piece_count_kernel(int nrow, int split, const int *__restrict__ row_ptr, int *__restrict__ cnt)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > nrow) return;
  if (r == nrow) { cnt[r] = 0; return; }
  const int len = row_ptr[r + 1] - row_ptr[r];
  cnt[r] = len <= split ? 1 : (len + split - 1) / split;
}

__global__ void vrow_fill_kernel(int nrow, int split, const int *__restrict__ row_ptr, const int *__restrict__ vfirst,
                                 int *__restrict__ vrow_ptr)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > nrow) return;
  if (r == nrow) { vrow_ptr[vfirst[nrow]] = row_ptr[nrow]; return; }
  const int a = row_ptr[r], v0 = vfirst[r], k = vfirst[r + 1] - v0;
  for (int i = 0; i < k; ++i) vrow_ptr[v0 + i] = a + i * split;
}

// last index i in [0, n] with a[i] <= key (a non-decreasing, a[0] <= key)
__device__ __forceinline__ int last_le(const int *__restrict__ a, int n, int64_t key)
{
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo + 1) >> 1);
    if ((int64_t)a[mid] <= key) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// key of entry e = panel(virtual row) * J + band(col); a stable sort by key starting from CSR order leaves every
// (panel, band) tile ordered by virtual row and, inside a row, in CSR storage order.
__global__ void tile_key_kernel(int nvrow, int64_t nnz, int P, int W, int J, const int *__restrict__ vrow_ptr,
                                const int *__restrict__ panel_row, const int *__restrict__ cols,
                                int *__restrict__ vrows, unsigned *__restrict__ keys)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  const int v = last_le(vrow_ptr, nvrow, i);      // empty virtual rows share a start: take the last, non-empty one
  vrows[i] = v;
  const int p = last_le(panel_row, P, v);
  keys[i] = (unsigned)p * (unsigned)J + (unsigned)(cols[i] / W);
}

__global__ void tile_pack_kernel(int64_t nnz, int W, int J, int lcol_bits, const unsigned *__restrict__ skeys,
                                 const unsigned *__restrict__ perm, const int *__restrict__ vrows,
                                 const int *__restrict__ panel_row, const int *__restrict__ cols,
                                 const double *__restrict__ vals, unsigned *__restrict__ pk, double *__restrict__ vals_out)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  const unsigned src = perm[i];
  const unsigned key = skeys[i];
  const unsigned p = key / (unsigned)J, j = key % (unsigned)J;
  const unsigned lrow = (unsigned)(vrows[src] - panel_row[p]), lcol = (unsigned)(cols[src] - (int)j * W);
  pk[i] = (lrow << lcol_bits) | lcol;
  if (vals) vals_out[i] = vals[src];
}

__global__ void max_row_len_kernel(int nrow, const int *__restrict__ row_ptr, int *__restrict__ out)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  int len = r < nrow ? row_ptr[r + 1] - row_ptr[r] : 0;
  for (int m = 32; m > 0; m >>= 1) { const int o = __shfl_xor(len, m); len = o > len ? o : len; }
  // one atomic per wave on ONE address cost 1.8 ms for 10 M rows (156 K serialised atomics); a wave whose maximum is not above what is
  // already there has nothing to add -- on uniform rows all but the first few skip
  if ((threadIdx.x & 63) == 0 && len > __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out, len);
}

// virtual rows of A for rows longer than `split`: vrow_ptr (nvrow + 1 entry offsets), vfirst (first virtual row of
// every row) and the vector of virtual sums; the two device arrays are handed to the caller's structure at once so
// that its destructor releases them on every path
static int make_virtual_rows(const DeviceCsr &A, int split, hipStream_t s, Scratch<int> &vrow_ptr, int *nvrow_out,
                             int **vfirst_out, double **yv_out, int kw = 1)
{
  Scratch<int> cnt;
  Scratch<char> tmp;
  int nvrow = 0;
  FS_HIP(cnt.alloc((size_t)A.nrow + 1));
  FS_HIP(traced_malloc(vfirst_out, sizeof(int) * ((size_t)A.nrow + 1)));
  int *vfirst = *vfirst_out;
  hipLaunchKernelGGL(piece_count_kernel, dim3(grid_for((int64_t)A.nrow + 1)), dim3(256), 0, s, A.nrow, split, A.row_ptr,
                     cnt.p);
  FS_HIP(hipGetLastError());
  if (int rc = device_exclusive_scan(tmp, cnt.p, vfirst, (size_t)A.nrow + 1, s)) return rc;
  if (int rc = read_back(&nvrow, (const int *)vfirst + A.nrow, s)) return rc;
  FS_HIP(vrow_ptr.alloc((size_t)nvrow + 1));
  hipLaunchKernelGGL(vrow_fill_kernel, dim3(grid_for((int64_t)A.nrow + 1)), dim3(256), 0, s, A.nrow, split, A.row_ptr,
                     vfirst, vrow_ptr.p);
  FS_HIP(hipGetLastError());
  FS_HIP(traced_malloc(yv_out, sizeof(double) * (size_t)nvrow * (size_t)kw));
  *nvrow_out = nvrow;
  return FS_OK;
}

static int max_row_len(const DeviceCsr &A, hipStream_t s, int *out)
{
  if (A.max_row_len >= 0) { *out = A.max_row_len; return FS_OK; }       // (every candidate builder asks)
  Scratch<int> mx;
  FS_HIP(mx.alloc(1));
  FS_HIP(hipMemsetAsync(mx, 0, sizeof(int), s));
  hipLaunchKernelGGL(max_row_len_kernel, dim3(grid_for(A.nrow)), dim3(256), 0, s, A.nrow, A.row_ptr, mx.p);
  FS_HIP(hipGetLastError());
  if (int rc = read_back(out, (const int *)mx.p, s)) return rc;
  A.max_row_len = *out;
  return FS_OK;
}

// The rows both builders work on: A's own, or -- when some row is longer than the split -- its virtual rows.
struct VirtualRows {
  Scratch<int> own;              // the virtual rows' entry offsets, when rows were cut
  const int *vrow_ptr = nullptr; // nvrow + 1 entry offsets (A.row_ptr when no row was cut)
  int nvrow = 0;
  int split = 0;                 // 0: no row was cut
  bool cut() const { return split > 0; }
  // the offsets on the host (the panels of cut rows are planned from them)
  int fetch(std::vector<int> &vp, hipStream_t s) const
  {
    vp.resize((size_t)nvrow + 1);
    FS_HIP(hipMemcpyAsync(vp.data(), vrow_ptr, sizeof(int) * vp.size(), hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
  }
};

// may_cut: the LDS-staged kernel balances by chunks of work items instead.  vfirst / yv are the copy's own slots.
static int virtual_rows(const DeviceCsr &A, hipStream_t s, bool may_cut, int kw, VirtualRows &V, int **vfirst, double **yv)
{
  int max_len = 0;
  if (int rc = max_row_len(A, s, &max_len)) return rc;
  const int split = options().tile_split > 0 ? options().tile_split : 256;
  V.vrow_ptr = A.row_ptr;
  V.nvrow = A.nrow;
  if (may_cut && max_len > split) {
    V.split = split;
    if (int rc = make_virtual_rows(A, split, s, V.own, &V.nvrow, vfirst, yv, kw)) return rc;
    V.vrow_ptr = V.own.p;
  }
  return FS_OK;
}

// The keys of all entries are computed (keys, in CSR order): sorts them stably with the entry indices between the two
// buffer pairs and finds the runs -- sorted_keys / perm point at the buffers that hold the result, run_ptr[k] = first
// sorted position of key k (nruns + 1 values).
static int sorted_runs(Scratch<char> &tmp, unsigned *keys, unsigned *skeys, unsigned *idx_in, unsigned *idx_out, size_t n, int64_t nruns,
                       int *run_ptr, hipStream_t s, const unsigned **sorted_keys, const unsigned **perm)
{
  if (int rc = device_iota((int64_t)n, idx_in, s)) return rc;
  if (int rc = device_sort_pairs(tmp, keys, skeys, idx_in, idx_out, n, sort_bits((uint64_t)nruns, 32), s, sorted_keys, perm)) return rc;
  return device_run_ptr(nruns, (int64_t)n, *sorted_keys, run_ptr, s);
}

// LDS-staged kernel only: inside a work item the order of the entries is free (the kernel adds with LDS atomics), so
// every item is rearranged for the LDS banks.  A half-wave (32 lanes) of the kernel takes 32 consecutive members of a
// SEQUENCE built here; its ds_add_f64 into the y slice is conflict-free when the 32 local rows differ mod 32 (bank pairs),
// its ds_read_b64 from the x slice when the 32 local columns differ mod 32.
//   Rows: round-robin over the row classes (local row mod 32) -- round r holds one entry of every class that still has
//     one, in class order, so lane l of a half-wave adds into bank pair l until the classes start to run out.
//   Columns (ARRANGE; FS_LDSX_ARRANGE=0 turns it off): WHICH entry of its class goes into round r is free.  The classes
//     of a round choose together so that their column banks differ: every class proposes a bank it still has entries for
//     and that the round has not used (starting from the diagonal (class + round) mod 32), the lowest class wins a
//     contested bank, the losers propose again; a class left without a free bank takes any.  Random columns cost 3.5
//     cycles per half-wave gather in stored order and about 2 this way (simulated).  Measured on config 3 with a serial
//     greedy of the same quality (which took 570 ms per matrix; this one works a round with 32 lanes at once):
//     A 0.79 -> 0.745 ms, A' 0.866 -> 0.824 ms.
// Sequence place s goes to stored position 2s (first half) or 2(s - half) + 1: the kernel's thread t takes the ADJACENT
// entries 2t and 2t + 1 (one 8-byte load), so the lanes of a wave see, for their first entry, every other stored
// position, and each of the two adds of a wave walks consecutive members of the sequence.
__device__ __forceinline__ int rot_ffs(unsigned m, int rot)   // lowest set bit of m at or after bit `rot`, cyclically (m != 0)
{
  const unsigned rr = rot ? ((m >> rot) | (m << (32 - rot))) : m;
  return (__ffs((int)rr) - 1 + rot) & 31;
}

// orders the LDS accesses of the lanes of ONE wave (the hardware runs a wave's LDS instructions in order; this keeps the
// compiler from moving them across and waits for the ones in flight)
__device__ __forceinline__ void wave_lds_fence()
{
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

constexpr int kReorderThreads = 256;
constexpr int kReorderSegs = kReorderThreads / 32;               // the item is counted in 8 segments at once
constexpr int kReorderPer = kTiledItem / kReorderThreads;        // entries per thread when the item is copied out

// Fixed-order sums (TiledCsr::orderable): a half of the sequence of 64 places is what ONE wave of the kernel adds with one
// instruction (thread = stored position / 2, wave = thread / 64), and a wave's LDS adds execute in program order.  So when all
// entries of a row inside an item sit with one wave, the row's y slot receives them in a fixed order whatever the other waves do.
// Rows with more than one entry in an item are few (config 3: 1 700 entries over 13 000 rows, ~110 of them) -- after the
// rounds, every such row is brought together: its entries swap places with single-entry rows of the same class (the class
// decides the LDS bank, so the bank arrangement of the rows is untouched; the column banks of the swapped pair change).
// *bad counts the items where that was not possible (a row with more entries than a wave has places for its class, a class
// too large to search): fixed-order products then leave this copy alone.
constexpr int kRepairMaxClass = 256;   // entries of one class the repair searches (2048 / 32 = 64 on average)
constexpr int kRepairMaxGroup = 8;     // entries of one row inside an item the per-class pass handles
constexpr int kRepairMaxLeft = 128;    // rows of an item left to the any-class pass
constexpr int kRepairMaxBig = 96;      // entries of one row inside an item at most (a wave holds 128 entries of an item)

template <bool ARRANGE>
__global__ __launch_bounds__(kReorderThreads) void ldsx_reorder_kernel(const int4 *__restrict__ items, int lcol_bits,
                                                                      unsigned *__restrict__ pk, double *__restrict__ vals,
                                                                      int *__restrict__ bad, unsigned long long *__restrict__ clk)
{
  // clk (FS_LDSX_REORDER_PROFILE=1, else nullptr): core clocks of thread 0 per phase, summed over the workgroups -- [0] load + count,
  // [1] prefixes + lists, [2] the rounds (wave 0), [3] repair: rows and leaders, [4] repair per class, [5] repair of what is left,
  // [6] copy out
  long long tick = clk ? clock64() : 0;
  auto lap = [&](int phase) {
    if (clk && threadIdx.x == 0) { const long long now = clock64(); atomicAdd(&clk[phase], (unsigned long long)(now - tick)); tick = now; }
  };
  __shared__ unsigned w[kTiledItem];
  __shared__ unsigned short lst[kTiledItem];   // entries grouped by (row class, column bank), stored order inside a group
  __shared__ unsigned short seq[kTiledItem];   // first: rank of an entry inside its (segment, class, bank); then the sequence
  __shared__ unsigned short segcnt[kReorderSegs][32 * 32];   // entries of (class, bank) per segment, then their prefix
  __shared__ unsigned short left[32 * 32];     // entries of (class, bank) not placed yet
  __shared__ unsigned short size[32 * 32];     // entries of (class, bank)
  __shared__ unsigned short off[32 * 32];      // first entry of (class, bank) in lst
  __shared__ int owner[32];
  // the repair: per class (entries of class c are indices off[c * 32] .. of these arrays, in round order).  They live in the
  // storage of segcnt, which is dead once lst is filled (with 14 KiB more LDS only two workgroups fit a CU instead of four, and
  // the kernel took twice as long: 219 -> 458 ms on config 3)
  static_assert(kReorderSegs * 32 * 32 >= 3 * kTiledItem + kTiledItem / 2, "the repair arrays are carved out of segcnt");
  unsigned short *const cplace = &segcnt[0][0];                   // place in the sequence
  unsigned short *const crow = &segcnt[0][0] + kTiledItem;        // local row
  unsigned short *const lead = &segcnt[0][0] + 2 * kTiledItem;    // first index of the class with the same row
  unsigned char *const flag = reinterpret_cast<unsigned char *>(&segcnt[0][0] + 3 * kTiledItem);   // bit 0: a leader whose row has
                                                                  // further entries; bit 1: placed for good
  __shared__ unsigned short unres[kRepairMaxLeft]; // leaders of the rows the per-class pass could not bring together
  __shared__ unsigned short pmem[kRepairMaxBig];  // the entries of one such row
  __shared__ int nunres, ndup, wcount[32];
  const int4 d = items[blockIdx.x];
  const int n = d.y, t = threadIdx.x;
  for (int i = t; i < n; i += kReorderThreads) w[i] = pk[(int64_t)d.x + i];
  for (int i = t; i < kReorderSegs * 32 * 32; i += kReorderThreads) (&segcnt[0][0])[i] = 0;
  __syncthreads();
  // thread (segment, class) walks its segment of the item and ranks the entries of its class per column bank
  {
    const int sg = t >> 5, c = t & 31;
    const int per = (n + kReorderSegs - 1) / kReorderSegs;
    const int i0 = sg * per, i1 = (i0 + per < n) ? i0 + per : n;
    for (int i = i0; i < i1; ++i)
      if ((int)((w[i] >> lcol_bits) & 31u) == c) {
        const int k = c * 32 + (ARRANGE ? (int)(w[i] & 31u) : 0);
        seq[i] = segcnt[sg][k]++;
      }
  }
  __syncthreads();
  lap(0);
  // per (class, bank): prefix over the segments, total
  for (int k = t; k < 32 * 32; k += kReorderThreads) {
    int a = 0;
    for (int sg = 0; sg < kReorderSegs; ++sg) { const int m = segcnt[sg][k]; segcnt[sg][k] = (unsigned short)a; a += m; }
    size[k] = (unsigned short)a;
    left[k] = (unsigned short)a;
  }
  __syncthreads();
  // lane c of wave 0 owns row class c: offsets of its banks in lst (class totals by a wave scan)
  unsigned avail = 0;                           // banks this class still has entries for
  int mine = 0;
  if (t < 64) {
    if (t < 32)
      for (int b = 0; b < 32; ++b) mine += size[t * 32 + b];
    int base = mine;
    for (int m = 1; m < 32; m <<= 1) {
      const int o = __shfl_up(base, m);
      if (t >= m) base += o;
    }
    base -= mine;
    if (t < 32) {
      int a = base;
      for (int b = 0; b < 32; ++b) {
        off[t * 32 + b] = (unsigned short)a;
        a += size[t * 32 + b];
        if (size[t * 32 + b]) avail |= 1u << b;
      }
    }
  }
  __syncthreads();
  {
    const int per = (n + kReorderSegs - 1) / kReorderSegs;
    for (int i = t; i < n; i += kReorderThreads) {
      const int k = (int)((w[i] >> lcol_bits) & 31u) * 32 + (ARRANGE ? (int)(w[i] & 31u) : 0);
      lst[off[k] + segcnt[i / per][k] + seq[i]] = (unsigned short)i;
    }
  }
  __syncthreads();
  lap(1);
  if (t < 64) {                                 // the rounds: wave 0, lanes 32-63 only take part in the ballots
    int remaining = t < 32 ? mine : 0, placed = 0;
    for (int r = 0;; ++r) {
      const unsigned nonempty = (unsigned)__ballot(remaining > 0);
      if (!nonempty) break;
      unsigned used = 0;
      int bank = -1;
      bool pending = remaining > 0;
      for (int iter = 0;; ++iter) {
        int prop = -1;
        if (pending) {
          const unsigned free_banks = avail & ~used;
          const int rot = (t + r + 7 * iter) & 31;
          if (!ARRANGE || free_banks == 0u) { bank = rot_ffs(avail, rot); pending = false; }
          else prop = rot_ffs(free_banks, rot);
        }
        if (!__ballot(prop >= 0)) break;        // everybody is settled
        if (t < 32) owner[t] = 255;
        wave_lds_fence();
        if (prop >= 0) atomicMin(&owner[prop], t);
        wave_lds_fence();
        if (prop >= 0 && owner[prop] == t) { bank = prop; pending = false; }
        used |= (unsigned)__ballot(t < 32 && owner[t & 31] != 255);    // lane index = bank index
        wave_lds_fence();
      }
      if (bank >= 0) {
        const int k = t * 32 + bank;
        const int before = left[k];
        left[k] = (unsigned short)(before - 1);
        if (before == 1) avail &= ~(1u << bank);
        const int place = placed + __popc(nonempty & ((1u << t) - 1u));
        seq[place] = lst[off[k] + (size[k] - before)];
        cplace[off[t * 32] + (mine - remaining)] = (unsigned short)place;
        --remaining;
      }
      placed += __popc(nonempty);
    }
  }
  __syncthreads();
  lap(2);
  const int half = (n + 1) >> 1;
  // ---- the repair: the entries of a row with one wave ----------------------------------------------------------------------
  {
    // (a) every index: its row, and the first index of its class with the same row
    for (int g = t; g < n; g += kReorderThreads) crow[g] = (unsigned short)(w[seq[cplace[g]]] >> lcol_bits);
    __syncthreads();
    bool too_large = false;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    auto rdlane = [](int v, int l) { return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(l)); };
    // wave wv takes the classes 8 wv .. 8 wv + 7, one after the other, 64 entries of the class with its lanes at a time: the rows
    // travel between the lanes through v_readlane (a thread per entry scanning its class in LDS was 83 K of the kernel's clocks)
    for (int q8 = 0; q8 < 8; ++q8) {
      const int c = wv * 8 + q8;
      // (wave-uniform values read from LDS: said so, or the loops over a class run under exec masks with their counters in VGPRs --
      // that alone was 70 K clocks per item)
      const int base = __builtin_amdgcn_readfirstlane((int)off[c * 32]);
      const int msize = __builtin_amdgcn_readfirstlane((c < 31 ? (int)off[(c + 1) * 32] : n) - base);
      const int m = msize < kRepairMaxClass ? msize : kRepairMaxClass;
      int row[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int idx = 64 * e + lane;
        row[e] = idx < m ? (int)crow[base + idx] : -1 - idx;              // (no row is negative: a lane outside the class matches nothing)
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (64 * e < m) {
          int first = -1;                                                  // place in the class of the first earlier entry of this row
#pragma unroll
          for (int e2 = 0; e2 < 4; ++e2) {
            if (e2 <= e) {
              const int lim = e2 < e ? 64 : lane;
              const int cnt = m - 64 * e2 < 64 ? m - 64 * e2 : 64;
              for (int l = 0; l < cnt; ++l) {
                const int rl = rdlane(row[e2], l);
                if (first < 0 && rl == row[e] && l < lim) first = 64 * e2 + l;
              }
            }
          }
          const int idx = 64 * e + lane;
          if (idx < m) {
            lead[base + idx] = (unsigned short)(base + (first < 0 ? idx : first));
            flag[base + idx] = 0;
          }
        }
      }
      for (int idx = kRepairMaxClass + lane; idx < msize; idx += 64) {     // a class beyond what the repair searches
        lead[base + idx] = (unsigned short)(base + idx);
        flag[base + idx] = 0;
        too_large = true;
      }
    }
    __syncthreads();
    if (t == 0) { nunres = 0; ndup = 0; }
    __syncthreads();
    {
      int mydup = 0;
      for (int g = t; g < n; g += kReorderThreads)
        if (lead[g] != g) { flag[lead[g]] = 1; ++mydup; }          // (several writers, one value)
      if (mydup) atomicAdd(&ndup, mydup);
    }
    __syncthreads();
    // an item in which every fourth entry repeats a row (dense rows: long rows of a short panel) is not worth the search: the
    // copy then simply has no fixed-order form
    lap(3);
    const bool hopeless = 4 * ndup > n && n > 128;   // (up to 128 entries all sit with wave 0 anyway)
    // (b) lane c of wave 0 brings the rows of class c together, one after the other, trading places with single-entry rows of
    // the SAME class only (the lanes work on disjoint lists); what does not fit that way goes on the list of (c)
    bool failed = too_large || hopeless;
    auto wave_of = [&](int g) { const int sp = cplace[g]; return (sp < half ? sp : sp - half) >> 6; };
    auto trade = [&](int j, int k, int g) {                     // member at index j <-> single-entry row at index k
      const unsigned short ej = seq[cplace[j]], ek = seq[cplace[k]];
      seq[cplace[j]] = ek; seq[cplace[k]] = ej;
      const unsigned short rj = crow[j]; crow[j] = crow[k]; crow[k] = rj;
      lead[k] = (unsigned short)g; flag[k] = 2;                  // the member now lives at k, for good
      lead[j] = (unsigned short)j; flag[j] = 0;                  // j holds the single-entry row
    };
    // Wave wv takes the classes 8 wv .. 8 wv + 7 one after the other with its lanes holding the class's entries (four per lane:
    // up to kRepairMaxClass): which row is next, who its members are, which wave holds most of them and where that wave has a free
    // single-entry row are BALLOTS over the lanes, a handful of instructions each, where one lane per class used to walk 64-entry
    // lists in LDS (0.28 M of the kernel's 0.59 M clocks per item).  Same choices as that serial form, so the same arrangement:
    // rows in ascending leader order, the wave that holds most members (the lowest on a tie), free rows lowest index first.
    if (!hopeless) {
      for (int q8 = 0; q8 < 8; ++q8) {
        const int c = wv * 8 + q8;
        const int base = __builtin_amdgcn_readfirstlane((int)off[c * 32]);
        const int msize = __builtin_amdgcn_readfirstlane((c < 31 ? (int)off[(c + 1) * 32] : n) - base);
        const int m = msize < kRepairMaxClass ? msize : kRepairMaxClass;
        if (m <= 0) continue;
        int wof[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) wof[e] = 64 * e + lane < m ? wave_of(base + 64 * e + lane) : 31;
        int myfree = 0;                                              // lane v < 16: free single-entry rows of this class with wave v
        {
          bool fr[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int g = base + 64 * e + lane;
            fr[e] = 64 * e + lane < m && lead[g] == g && !(flag[g] & 3);
          }
          for (int v = 0; v < 16; ++v) {
            int cnt = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) cnt += __popcll(__ballot(fr[e] && wof[e] == v));
            if (lane == v) myfree = cnt;
          }
        }
        int cursor = -1;                                             // place in the class of the last row handled
        for (;;) {
          int G = -1;                                                // the next leader of a row with several entries
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int idx = 64 * e + lane, g = base + idx;
            const bool d = idx < m && idx > cursor && lead[g] == g && (flag[g] & 1) && !(flag[g] & 2);
            const unsigned long long mk = __ballot(d);
            if (G < 0 && mk) G = 64 * e + __ffsll((long long)mk) - 1;
          }
          if (G < 0) break;
          cursor = G;
          const int gG = base + G;
          bool mem[4];
          int gs = 0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            mem[e] = 64 * e + lane < m && lead[base + 64 * e + lane] == gG;
            gs += __popcll(__ballot(mem[e]));
          }
          int best = -1;
          if (gs <= kRepairMaxGroup) {
            int have = 0;                                            // lane v < 16: members already with wave v
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              unsigned long long bits = __ballot(mem[e]);
              while (bits) {
                const int l = __ffsll((long long)bits) - 1;
                bits &= bits - 1;
                if (lane == rdlane(wof[e], l)) ++have;
              }
            }
            int key = (lane < 16 && have + myfree >= gs) ? ((have << 8) | (15 - lane)) : -1;   // most members; the lowest wave on a tie
            for (int o = 32; o > 0; o >>= 1) { const int other = __shfl_xor(key, o); key = other > key ? other : key; }
            if (key >= 0) best = 15 - (key & 255);
          }
          if (best < 0) {                                            // too many entries, or no wave with room: left to (c)
            if (lane == 0) {
              const int slot = atomicAdd(&nunres, 1);
              if (slot < kRepairMaxLeft) unres[slot] = (unsigned short)gG; else failed = true;
            }
            continue;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            unsigned long long bits = __ballot(mem[e]);
            while (bits) {
              const int l = __ffsll((long long)bits) - 1;
              bits &= bits - 1;
              const int j = base + 64 * e + l;
              const int wj = rdlane(wof[e], l);
              if (wj == best) {
                if (lane == 0) flag[j] |= 2;
                wave_lds_fence();
                continue;
              }
              int k = -1;                                            // the lowest free single-entry row with that wave
#pragma unroll
              for (int e2 = 0; e2 < 4; ++e2) {
                const int g2 = base + 64 * e2 + lane;
                const bool f = 64 * e2 + lane < m && wof[e2] == best && lead[g2] == g2 && !(flag[g2] & 3);
                const unsigned long long fm = __ballot(f);
                if (k < 0 && fm) k = base + 64 * e2 + __ffsll((long long)fm) - 1;
              }
              if (k < 0) { failed = true; break; }                   // (cannot happen: myfree counted it)
              if (lane == 0) trade(j, k, gG);
              wave_lds_fence();
              if (lane == best) --myfree;
              if (lane == wj) ++myfree;                              // j now holds the single-entry row
            }
          }
          wave_lds_fence();
        }
      }
    }
    __syncthreads();
    // the rows left to (c) in ascending order whichever wave listed them first: the arrangement must not depend on timing
    {
      const int cnt = nunres < kRepairMaxLeft ? nunres : kRepairMaxLeft;
      int mine_u = 0, rank = 0;
      if (t < cnt) {
        mine_u = unres[t];
        for (int j = 0; j < cnt; ++j) rank += unres[j] < mine_u;
      }
      __syncthreads();
      if (t < cnt) unres[rank] = (unsigned short)mine_u;
    }
    __syncthreads();
    lap(4);
    // (c) what is left -- rows with more entries than a wave has places for their class, or an unlucky packing -- trades places
    // with single-entry rows of ANY class of the chosen wave (a few lanes of that wave then share a bank: rare).  One row after
    // the other; the whole workgroup counts the members and the free single-entry rows per wave, thread 0 chooses and trades.
    {
      const int left = hopeless ? 0 : (nunres < kRepairMaxLeft ? nunres : kRepairMaxLeft);    // (uniform: nunres is in LDS)
      if (!hopeless && nunres > kRepairMaxLeft) failed = true;
      for (int u = 0; u < left; ++u) {
        const int g = unres[u];
        if (t < 32) wcount[t] = 0;                               // [0, 16): members per wave, [16, 32): free single-entry rows
        __syncthreads();
        for (int j = t; j < n; j += kReorderThreads) {
          const int v = wave_of(j);
          if (lead[j] == g) atomicAdd(&wcount[v], 1);
          else if (lead[j] == j && !(flag[j] & 3)) atomicAdd(&wcount[16 + v], 1);
        }
        __syncthreads();
        if (t == 0 && !failed) {
          const int c = crow[g] & 31, base = off[c * 32];
          int m = (c < 31 ? (int)off[(c + 1) * 32] : n) - base;
          if (m > kRepairMaxClass) m = kRepairMaxClass;
          int gs = 0;
          for (int j = g; j < base + m; ++j)
            if (lead[j] == g) { if (gs < kRepairMaxBig) pmem[gs] = (unsigned short)j; ++gs; }
          int best = -1;                                         // the wave that already holds most of the row, among those with room
          for (int v = 0; v < 16; ++v)
            if (wcount[v] + wcount[16 + v] >= gs && (best < 0 || wcount[v] > wcount[best])) best = v;
          if (gs > kRepairMaxBig || best < 0) failed = true;
          else {
            int next = 0;
            for (int q = 0; q < gs; ++q) {
              const int j = pmem[q];
              if (wave_of(j) == best) { flag[j] |= 2; continue; }
              while (next < n && !(wave_of(next) == best && lead[next] == next && !(flag[next] & 3))) ++next;
              if (next >= n) { failed = true; break; }
              trade(j, next, g);
            }
          }
        }
        __syncthreads();
      }
    }
    if (failed) atomicAdd(bad, 1);
  }
  __syncthreads();
  lap(5);
  // copy out: sources into registers first (the item is permuted in place)
  double v[kReorderPer];
#pragma unroll
  for (int j = 0; j < kReorderPer; ++j) {
    const int q = t + j * kReorderThreads;
    v[j] = (vals && q < n) ? vals[(int64_t)d.x + seq[q]] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kReorderPer; ++j) {
    const int q = t + j * kReorderThreads;
    if (q < n) {
      const int pos = q < half ? 2 * q : 2 * (q - half) + 1;
      pk[(int64_t)d.x + pos] = w[seq[q]];
      if (vals) vals[(int64_t)d.x + pos] = v[j];
    }
  }
  lap(6);
}

// how many column bands of W columns do the entries of panel (blockIdx.x * stride) touch?  out[2b] = bands, out[2b + 1] = entries
constexpr int kPanelBandWords = 8192;    // 262 144 bands: 32 KiB of LDS
__global__ __launch_bounds__(256) void panel_bands_kernel(int stride, int W, int words, const int *__restrict__ panel_row,
                                                          const int *__restrict__ row_ptr, const int *__restrict__ cols,
                                                          int *__restrict__ out)
{
  __shared__ unsigned bits[kPanelBandWords];
  __shared__ int total;
  const int p = blockIdx.x * stride, t = threadIdx.x;
  for (int i = t; i < words; i += 256) bits[i] = 0u;
  if (t == 0) total = 0;
  __syncthreads();
  const int64_t e0 = row_ptr[panel_row[p]], e1 = row_ptr[panel_row[p + 1]];
  for (int64_t e = e0 + t; e < e1; e += 256) {
    const int b = cols[e] / W;
    atomicOr(&bits[b >> 5], 1u << (b & 31));
  }
  __syncthreads();
  int c = 0;
  for (int i = t; i < words; i += 256) c += __popc(bits[i]);
  atomicAdd(&total, c);
  __syncthreads();
  if (t == 0) { out[2 * blockIdx.x] = total; out[2 * blockIdx.x + 1] = (int)(e1 - e0); }
}

// auto mode, LDS-staged copy with thin tiles on average: the bands a sample of panels really touches (ldsx_sample_thin)
static int ldsx_sample_is_thin(const DeviceCsr &A, const int *vrow_ptr, const std::vector<int> &panel_row, int W, int J, hipStream_t s,
                               bool *thin)
{
  *thin = true;
  constexpr int kSample = 64;
  const int P = (int)panel_row.size() - 1, words = (J + 31) / 32;
  if (words > kPanelBandWords || P < 1) return FS_OK;
  const int ns = P < kSample ? P : kSample, stride = P / ns;
  Scratch<int> prow, cnt;
  FS_HIP(prow.alloc(panel_row.size()));
  FS_HIP(cnt.alloc(2 * (size_t)ns));
  FS_HIP(hipMemcpyAsync(prow.p, panel_row.data(), sizeof(int) * panel_row.size(), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(panel_bands_kernel, dim3(ns), dim3(256), 0, s, stride, W, words, prow.p, vrow_ptr, A.cols, cnt.p);
  FS_HIP(hipGetLastError());
  std::vector<int> hc(2 * (size_t)ns);
  FS_HIP(hipMemcpyAsync(hc.data(), cnt.p, sizeof(int) * hc.size(), hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  *thin = ldsx_sample_thin(hc);
  return FS_OK;
}

// LDS-staged copy: every work item arranged for the LDS banks (ldsx_reorder_kernel); T->orderable = every row of every item
// sits with one wave, so fixed-order sums are possible on this copy
static int reorder_ldsx_items(TiledCsr *T, hipStream_t s)
{
  static const bool arrange = [] { const char *v = getenv("FS_LDSX_ARRANGE"); return !(v && *v == '0'); }();
  static const bool profile = [] { const char *v = getenv("FS_LDSX_REORDER_PROFILE"); return v && *v == '1'; }();
  Scratch<int> bad;
  Scratch<unsigned long long> clk;
  FS_HIP(bad.alloc(1));
  FS_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
  if (profile) { FS_HIP(clk.alloc(8)); FS_HIP(hipMemsetAsync(clk, 0, 8 * sizeof(unsigned long long), s)); }
  if (arrange)
    hipLaunchKernelGGL(ldsx_reorder_kernel<true>, dim3(T->nitems), dim3(kReorderThreads), 0, s, T->items, T->lcol_bits, T->pk, T->vals, bad.p, profile ? clk.p : nullptr);
  else
    hipLaunchKernelGGL(ldsx_reorder_kernel<false>, dim3(T->nitems), dim3(kReorderThreads), 0, s, T->items, T->lcol_bits, T->pk, T->vals, bad.p, profile ? clk.p : nullptr);
  FS_HIP(hipGetLastError());
  if (profile) {
    unsigned long long h[8] = {};
    FS_HIP(hipMemcpyAsync(h, clk, sizeof h, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    fprintf(stderr, "[fastsparse] ldsx_reorder_kernel, %d items, mean clocks per item: load+count %.0f, lists %.0f, rounds %.0f, repair rows+leaders %.0f, "
            "per class %.0f, leftovers %.0f, copy out %.0f\n", T->nitems, (double)h[0] / T->nitems, (double)h[1] / T->nitems, (double)h[2] / T->nitems,
            (double)h[3] / T->nitems, (double)h[4] / T->nitems, (double)h[5] / T->nitems, (double)h[6] / T->nitems);
  }
  int hbad = 0;
  if (int rc = read_back(&hbad, bad.p, s)) return rc;
  T->orderable = hbad == 0;                       // every row of every item with one wave: fixed-order sums possible
  if (trace_build() && hbad) fprintf(stderr, "[fastsparse] LDS-staged copy: %d of %d work items hold a row that does not fit one wave -- no fixed-order sums on this copy\n", hbad, T->nitems);
  return FS_OK;
}

// the chunk tables of the LDS-staged copy, their tickets and -- when chunks share a panel -- the zeroed scratch vector
static int upload_ldsx_chunks(TiledCsr *T, int nrow, const std::vector<int> &chunk_panel, const std::vector<int> &chunk_item,
                              const std::vector<int> &chunk_ord)
{
  const int P = T->P;
  T->nchunks = (int)chunk_panel.size();
  FS_HIP(traced_malloc(&T->chunk_panel, sizeof(int) * (chunk_panel.size() ? chunk_panel.size() : 1)));
  FS_HIP(traced_malloc(&T->chunk_item, sizeof(int) * (chunk_item.size() ? chunk_item.size() : 2)));
  FS_HIP(traced_malloc(&T->chunk_ord, sizeof(int) * (chunk_ord.size() ? chunk_ord.size() : 1)));
  {   // ticket[-1]: chunks that gave up waiting for their turn (ldsx_store_slice), ever; ticket[0 .. P): whose turn it is
    int *base = nullptr;
    FS_HIP(traced_malloc(&base, sizeof(int) * ((size_t)(P > 0 ? P : 1) + 1)));
    FS_HIP(hipMemset(base, 0, sizeof(int)));
    T->ticket = base + 1;
  }
  if (!chunk_panel.empty()) {
    FS_HIP(hipMemcpy(T->chunk_panel, chunk_panel.data(), sizeof(int) * chunk_panel.size(), hipMemcpyHostToDevice));
    FS_HIP(hipMemcpy(T->chunk_item, chunk_item.data(), sizeof(int) * chunk_item.size(), hipMemcpyHostToDevice));
    FS_HIP(hipMemcpy(T->chunk_ord, chunk_ord.data(), sizeof(int) * chunk_ord.size(), hipMemcpyHostToDevice));
  }
  if (T->shared && !T->yv) FS_HIP(traced_malloc(&T->yv, sizeof(double) * (size_t)nrow));
  return FS_OK;
}

static int build_tiled_impl(DeviceCsr &A, hipStream_t s, TiledCsr *&slot, bool ldsx)
{
  const Options &o = options();
  const int mode = ldsx ? o.ldsx : o.tiling;   // 0 never, 1 when the estimates do not rule it out, 2 always
  if (mode == 0 || A.nrow == 0 || A.nnz == 0) return FS_OK;
  const int ncu = cu_count();
  const int slots = (ncu > 8 ? ncu : 256) / 8 * 8;  // one workgroup per CU, a multiple of the 8 XCDs
  const int rows_max = ldsx ? kLdsxRows : kTiledRowsMax;

  // ---- cheap rejections first (auto mode) ----------------------------------------------------------
  const int64_t x_bytes = (int64_t)A.ncol * 8;
  if (mode == 1 && tiled_too_small(x_bytes, A.nnz)) return FS_OK;

  // ---- virtual rows ------------------------------------------------------------------------------------
  TiledCsr *T = new TiledCsr();
  slot = T;
  T->ldsx = ldsx;
  T->slots = slots; T->lcol_bits = kTiledColBits;
  VirtualRows V;
  if (int rc = virtual_rows(A, s, !ldsx, 1, V, &T->vfirst, &T->yv)) return rc;
  T->split = V.split;
  T->nvrow = V.nvrow;

  // ---- plan: panels and band width (fs_plan.h), then what the estimates say about them ---------------------
  const int R = plan_tiled_rows(V.nvrow, slots, rows_max, ldsx, o.tile_rows);
  std::vector<int> vp;
  if (V.cut())
    if (int rc = V.fetch(vp, s)) return rc;
  const std::vector<int> panel_row = plan_tiled_panels(V.nvrow, R, V.cut(), vp, A.nnz, V.split);
  const int P = (int)panel_row.size() - 1;
  int W = 0, J = 0;
  plan_band_width(A.ncol, A.nnz, P, ldsx, o.tile_cols, &W, &J);
  const int64_t ntiles = (int64_t)P * J;
  if (mode == 1 && ldsx && ldsx_tiles_thin(A.nnz, ntiles)) {
    bool thin = true;
    if (int rc = ldsx_sample_is_thin(A, V.vrow_ptr, panel_row, W, J, s, &thin)) return rc;
    if (thin) return FS_OK;
  }
  if (mode == 1 && !ldsx && tiled_hopeless(A.nnz, ntiles, P, slots, x_bytes)) return FS_OK;
  if (ntiles >= (1ll << 31)) return FS_OK;
  T->R = R; T->W = W; T->P = P; T->J = J;
  T->entries_per_tile = (float)((double)A.nnz / (double)ntiles);
  FS_HIP(traced_malloc(&T->panel_row, sizeof(int) * panel_row.size()));
  FS_HIP(hipMemcpyAsync(T->panel_row, panel_row.data(), sizeof(int) * panel_row.size(), hipMemcpyHostToDevice, s));

  // ---- sort the entries by (panel, band), pack them, cut the work items -----------------------------------
  const size_t n = (size_t)A.nnz;
  Scratch<int> vrows, tile_ptr;
  Scratch<unsigned> keys, skeys, idx_in, idx_out;
  Scratch<char> tmp;
  FS_HIP(vrows.alloc(n));
  FS_HIP(keys.alloc(n));
  FS_HIP(skeys.alloc(n));
  FS_HIP(idx_in.alloc(n));
  FS_HIP(idx_out.alloc(n));
  FS_HIP(tile_ptr.alloc((size_t)ntiles + 1));
  FS_HIP(traced_malloc(&T->pk, sizeof(unsigned) * (n + 8)));          // + slack: the LDS-staged kernel loads entries in pairs
  if (A.vals) FS_HIP(traced_malloc(&T->vals, sizeof(double) * (n + 8)));
  hipLaunchKernelGGL(tile_key_kernel, dim3(grid_for(A.nnz)), dim3(256), 0, s, V.nvrow, A.nnz, P, W, J, V.vrow_ptr, T->panel_row,
                     A.cols, vrows.p, keys.p);
  const unsigned *sorted_keys = nullptr, *perm = nullptr;
  if (int rc = sorted_runs(tmp, keys.p, skeys.p, idx_in.p, idx_out.p, n, ntiles, tile_ptr.p, s, &sorted_keys, &perm)) return rc;
  hipLaunchKernelGGL(tile_pack_kernel, dim3(grid_for(A.nnz)), dim3(256), 0, s, A.nnz, W, J, T->lcol_bits, sorted_keys, perm,
                     vrows.p, T->panel_row, A.cols, A.vals, T->pk, T->vals);
  FS_HIP(hipGetLastError());
  // work items are cut on the host from the tile pointers (P*J ints)
  std::vector<int> tp((size_t)ntiles + 1);
  FS_HIP(hipMemcpyAsync(tp.data(), tile_ptr.p, sizeof(int) * tp.size(), hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  std::vector<WorkItem> items;
  std::vector<int> item_ptr;
  cut_work_items(tp, P, J, items, item_ptr);
  T->nitems = (int)items.size();
  FS_HIP(traced_malloc(&T->items, sizeof(int4) * (items.size() ? items.size() : 1)));
  FS_HIP(traced_malloc(&T->item_ptr, sizeof(int) * item_ptr.size()));
  if (!items.empty()) FS_HIP(hipMemcpy(T->items, items.data(), sizeof(int4) * items.size(), hipMemcpyHostToDevice));
  FS_HIP(hipMemcpy(T->item_ptr, item_ptr.data(), sizeof(int) * item_ptr.size(), hipMemcpyHostToDevice));
  if (ldsx && T->nitems > 0)
    if (int rc = reorder_ldsx_items(T, s)) return rc;
  if (ldsx) {
    static const bool plain = [] { const char *v = getenv("FS_LDSX_ORDER"); return v && *v == '1'; }();
    std::vector<int> chunk_panel, chunk_item, chunk_ord;
    T->shared = plan_ldsx_chunks(item_ptr, (int64_t)items.size(), P, slots, plain, chunk_panel, chunk_item, chunk_ord);
    if (int rc = upload_ldsx_chunks(T, A.nrow, chunk_panel, chunk_item, chunk_ord)) return rc;
  }
  T->built = true;
  return FS_OK;
}

// The tiled copies are optimisations: if building one fails (typically: not enough HBM for another copy) the
// matrix stays usable on the other kernels.
int build_tiled(DeviceCsr &A, hipStream_t s) { return optional_copy(build_tiled_impl(A, s, A.tiled, false), A.tiled, free_tiled_slot); }

// the same layout with the geometry of the LDS-staged kernel (x slices of kLdsxCols columns)
int build_tiledx(DeviceCsr &A, hipStream_t s) { return optional_copy(build_tiled_impl(A, s, A.tiledx, true), A.tiledx, free_tiled_slot); }

// ---- two-pass copy ------------------------------------------------------------------------------------
// key of entry e = band(col) * P + panel(virtual row): a stable sort by key starting from CSR order leaves every
// (band, panel) run in CSR storage order
__global__ void bin_key_kernel(int nvrow, int64_t nnz, int P, int bcols, const int *__restrict__ vrow_ptr,
                               const int *__restrict__ panel_row, const int *__restrict__ cols,
                               int *__restrict__ vrows, unsigned *__restrict__ keys)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  const int v = last_le(vrow_ptr, nvrow, i);
  vrows[i] = v;
  keys[i] = (unsigned)(cols[i] / bcols) * (unsigned)P + (unsigned)last_le(panel_row, P, v);
}

// group counts of the padded runs in pass-1 order (g1[band*P + panel]) and pass-2 order (g2[panel*B + band]);
// slot nruns of both is the zero that turns the exclusive scans into B*P + 1 offsets
__global__ void bin_groups_kernel(int B, int P, int ge, const int *__restrict__ run_ptr, unsigned *__restrict__ g1,
                                  unsigned *__restrict__ g2, const unsigned *__restrict__ xs = nullptr)
{
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nruns = (int64_t)B * P;
  if (k > nruns) return;
  if (k == nruns) { g1[k] = 0; g2[k] = 0; return; }
  const int b = (int)(k / P), p = (int)(k % P);
  const unsigned dum = xs ? xs[run_ptr[k + 1]] - xs[run_ptr[k]] : 0u;                   // (one-byte row steps: the run's dummy entries)
  const unsigned g = ((unsigned)(run_ptr[k + 1] - run_ptr[k]) + dum + (unsigned)ge - 1u) / (unsigned)ge;   // ge entries per group
  g1[k] = g;
  g2[(int64_t)p * B + b] = g;
}

__global__ void bin_scatter_kernel(int64_t nnz, int B, int P, int bcols, int ge, const unsigned *__restrict__ skeys,
                                   const unsigned *__restrict__ perm, const int *__restrict__ vrows,
                                   const int *__restrict__ panel_row, const int *__restrict__ cols,
                                   const double *__restrict__ vals, const int *__restrict__ run_ptr,
                                   const unsigned *__restrict__ start1, const unsigned *__restrict__ start2,
                                   uint16_t *__restrict__ lcol, double *__restrict__ vals2, uint16_t *__restrict__ lrow)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  const unsigned key = skeys[i], src = perm[i];
  const int b = (int)(key / (unsigned)P), p = (int)(key % (unsigned)P);
  const int64_t rank = i - run_ptr[key];
  const int64_t pos1 = (int64_t)start1[key] * ge + rank;
  const int64_t pos2 = (int64_t)start2[(int64_t)p * B + b] * ge + rank;
  lcol[pos1] = (uint16_t)(cols[src] - b * bcols);
  if (vals) vals2[pos2] = vals[src];                             // the values travel with the row ids: pass 2 multiplies
  lrow[pos2] = (uint16_t)(vrows[src] - panel_row[p]);
}

// ---- one-byte row steps (BinnedCsr::lrow8) ----
// extra[i] = dummy entries in front of sorted entry i: its step from the entry before it in the same run, walked 255 rows at a time
// (the first entry of a run starts from its own row: no step).  extra[nnz] = 0 closes the scan.
__global__ void bin_gap_kernel(int64_t nnz, int P, const unsigned *__restrict__ skeys, const unsigned *__restrict__ perm,
                               const int *__restrict__ vrows, const int *__restrict__ run_ptr, unsigned *__restrict__ extra)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > nnz) return;
  if (i == nnz) { extra[i] = 0; return; }
  const unsigned key = skeys[i];
  unsigned e = 0;
  if (i > run_ptr[key]) {
    const int gap = vrows[perm[i]] - vrows[perm[i - 1]];       // same panel: the difference of the local rows
    if (gap > 255) e = (unsigned)(gap - 1) / 255u;
  }
  extra[i] = e;
}

// the scatter of both orders with the dummies in place: slot = rank in the run + the dummies in front of it
__global__ void bin_scatter8_kernel(int64_t nnz, int B, int P, int bcols, int ge, const unsigned *__restrict__ skeys,
                                    const unsigned *__restrict__ perm, const int *__restrict__ vrows,
                                    const int *__restrict__ panel_row, const int *__restrict__ cols,
                                    const double *__restrict__ vals, const int *__restrict__ run_ptr,
                                    const unsigned *__restrict__ xs, const unsigned *__restrict__ start1,
                                    const unsigned *__restrict__ start2, uint16_t *__restrict__ lcol, double *__restrict__ vals2,
                                    uint8_t *__restrict__ lrow8, uint16_t *__restrict__ gbase)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  const unsigned key = skeys[i], src = perm[i];
  const int b = (int)(key / (unsigned)P), p = (int)(key % (unsigned)P);
  const int64_t first = run_ptr[key];
  const unsigned dum = xs[i + 1] - xs[i];                       // dummies in front of this entry
  const int64_t slot = (i - first) + (int64_t)(xs[i] - xs[first]) + dum;
  const int64_t base1 = (int64_t)start1[key] * ge, base2 = (int64_t)start2[(int64_t)p * B + b] * ge;
  const int row = vrows[src] - panel_row[p];
  const int prev = i > first ? vrows[perm[i - 1]] - panel_row[p] : row;    // the row in front of the first slot of a run: its own
  // the dummies: zero slot of the band (lcol = bcols and vals = 0 are the arrays' fill), step 255 each
  for (unsigned m = 0; m < dum; ++m) {
    const int64_t sl = slot - dum + m;
    lrow8[base2 + sl] = 255;
    if ((sl & (ge - 1)) == 0) gbase[(base2 + sl) / ge] = (uint16_t)(prev + 255 * (int)m);
  }
  const int before = prev + 255 * (int)dum;
  lcol[base1 + slot] = (uint16_t)(cols[src] - b * bcols);
  if (vals) vals2[base2 + slot] = vals[src];
  lrow8[base2 + slot] = (uint8_t)(row - before);
  if ((slot & (ge - 1)) == 0) gbase[(base2 + slot) / ge] = (uint16_t)before;
}

// gdst[g] = pass-2 group of pass-1 group g (one thread per run walks the run's groups)
__global__ void bin_gdst_kernel(int B, int P, const unsigned *__restrict__ start1, const unsigned *__restrict__ start2,
                                unsigned *__restrict__ gdst)
{
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (int64_t)B * P) return;
  const int b = (int)(k / P), p = (int)(k % P);
  const unsigned a = start1[k], n = start1[k + 1] - a, d = start2[(int64_t)p * B + b];
  for (unsigned j = 0; j < n; ++j) gdst[a + j] = d + j;
}

// band_ptr[b] = first pass-1 group of band b (B + 1 values), bin_ptr[p] = first pass-2 group of panel p (P + 1)
__global__ void bin_ptr_kernel(int B, int P, const unsigned *__restrict__ start1, const unsigned *__restrict__ start2,
                               unsigned *__restrict__ band_ptr, unsigned *__restrict__ bin_ptr)
{
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k <= B) band_ptr[k] = start1[k * P];
  if (k <= P) bin_ptr[k] = start2[k * B];
}

// ---- the longest rows of a heavy-tailed matrix, outside the two-pass copy (LongRows, fs_common.h) -------------------------
__global__ void long_candidates_kernel(int nrow, int minlen, const int *__restrict__ row_ptr, int *__restrict__ count, int cap,
                                       int2 *__restrict__ out)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrow) return;
  const int len = row_ptr[r + 1] - row_ptr[r];
  if (len < minlen) return;
  const int k = atomicAdd(count, 1);
  if (k < cap) out[k] = make_int2(r, len);
}

__global__ void long_mark_kernel(int nlong, const int *__restrict__ rows, int *__restrict__ row_to_long)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nlong) row_to_long[rows[i]] = i;
}

__global__ void main_len_kernel(int nrow, const int *__restrict__ row_ptr, const int *__restrict__ row_to_long, int *__restrict__ len)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > nrow) return;
  len[r] = (r == nrow || row_to_long[r] >= 0) ? 0 : row_ptr[r + 1] - row_ptr[r];
}

// every entry goes either to its place in the CSR without the long rows or, as (key = band * nlong + long row, source index),
// to the list the long rows' copy is sorted from
__global__ void split_entries_kernel(int nrow, int64_t nnz, int nlong, int bcols, const int *__restrict__ row_ptr, const int *__restrict__ cols,
                                     const double *__restrict__ vals, const int *__restrict__ row_to_long,
                                     const int *__restrict__ main_rp, const int64_t *__restrict__ long_ptr,
                                     int *__restrict__ main_cols, double *__restrict__ main_vals, unsigned *__restrict__ lkey,
                                     unsigned *__restrict__ lsrc)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  const int r = last_le(row_ptr, nrow, i);
  const int64_t k = i - row_ptr[r];
  const int l = row_to_long[r];
  if (l < 0) {
    const int64_t d = (int64_t)main_rp[r] + k;
    main_cols[d] = cols[i];
    if (vals) main_vals[d] = vals[i];
  } else {
    const int64_t d = long_ptr[l] + k;
    lkey[d] = (unsigned)(cols[i] / bcols) * (unsigned)nlong + (unsigned)l;
    lsrc[d] = (unsigned)i;
  }
}

// first sorted entry of every (band, owner) segment: seg = b * kLongOwners + w starts at the first key >= b * nlong + own_first[w]
__global__ void long_seg_start_kernel(int B, int nlong, int64_t n, const int *__restrict__ own_first, const unsigned *__restrict__ skeys,
                                      int64_t *__restrict__ start)
{
  const int64_t sg = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (sg > (int64_t)B * kLongOwners) return;
  const int b = (int)(sg / kLongOwners), w = (int)(sg % kLongOwners);
  const uint64_t key = (uint64_t)b * (uint64_t)nlong + (uint64_t)(b < B ? own_first[w] : 0);
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((uint64_t)skeys[mid] < key) lo = mid + 1; else hi = mid;
  }
  start[sg] = lo;
}

// owner_of[l]: the owner of long row l; shift[seg]: padded position - sorted position of the segment's entries
__global__ void long_scatter_kernel(int64_t n, int nlong, int bcols, const unsigned *__restrict__ skeys, const unsigned *__restrict__ ssrc,
                                    const unsigned char *__restrict__ owner_of, const int64_t *__restrict__ shift,
                                    const int *__restrict__ cols, const double *__restrict__ vals, uint16_t *__restrict__ lcol,
                                    uint16_t *__restrict__ lrow, double *__restrict__ lvals)
{
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const unsigned key = skeys[k], src = ssrc[k];
  const unsigned b = key / (unsigned)nlong, l = key - b * (unsigned)nlong;
  const int64_t d = k + shift[(int64_t)b * kLongOwners + owner_of[l]];
  lcol[d] = (uint16_t)(cols[src] - (int)b * bcols);
  lrow[d] = (uint16_t)l;
  if (lvals) lvals[d] = vals[src];
}

// a segment with an odd number of entries ends in one padding entry: column = the zero slot, value 0, row = its neighbour's
__global__ void long_pad_kernel(int64_t nseg, int bcols, const int64_t *__restrict__ start, const int64_t *__restrict__ shift,
                                uint16_t *__restrict__ lcol, uint16_t *__restrict__ lrow, double *__restrict__ lvals)
{
  const int64_t sg = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (sg >= nseg) return;
  const int64_t cnt = start[sg + 1] - start[sg];
  if (cnt & 1) {
    const int64_t d = start[sg] + shift[sg] + cnt;
    lcol[d] = (uint16_t)bcols;
    lrow[d] = lrow[d - 1];
    if (lvals) lvals[d] = 0.0;
  }
}

// Takes the longest rows out: on success *out holds their copy and main_* a CSR of the same shape without their entries
// (temporaries of the caller's build).  *out stays NULL when the matrix has no such rows or they would not pay.
static int split_long_rows(const DeviceCsr &A, hipStream_t s, LongRows **out, Scratch<int> &main_rp, Scratch<int> &main_cols,
                           Scratch<double> &main_vals, int64_t *main_nnz)
{
  *out = nullptr;
  const Options &o = options();
  if (o.long_rows == 0 || o.binning == 0 || A.nrow == 0 || A.nnz < (4 << 20)) return FS_OK;
  // geometry: the narrow band with 12032 accumulators covers more entries (a config-5 shard: 50 % against 40 %) at twice the
  // number of band loads; measured on the config-5 shard: 2.24 ms against 2.29 (and 2.71 without this path), so it is the
  // default; long_geometry / FS_LONG_GEOMETRY force either
  const bool narrow = o.long_geometry != 1;
  const int bcols = narrow ? kLongBandB : kLongBandA, cap_rows = narrow ? kLongRowsB : kLongRowsA;
  const int B = (A.ncol + bcols - 1) / bcols;
  // ANY row saves its intermediate products here; what limits the path is the number of accumulators, so the longest rows
  // are taken.  Candidates: rows of at least 512 entries (shorter ones are too many to be worth collecting).
  const int minlen = o.long_min_len > 0 ? o.long_min_len : 512;
  constexpr int kCap = 1 << 18;
  Scratch<int> cnt;
  Scratch<int2> cand;
  FS_HIP(cnt.alloc(1));
  FS_HIP(cand.alloc(kCap));
  FS_HIP(hipMemsetAsync(cnt, 0, sizeof(int), s));
  hipLaunchKernelGGL(long_candidates_kernel, dim3(grid_for(A.nrow)), dim3(256), 0, s, A.nrow, minlen, A.row_ptr, cnt.p, kCap, cand.p);
  FS_HIP(hipGetLastError());
  int ncand = 0;
  if (int rc = read_back(&ncand, cnt.p, s)) return rc;
  if (ncand == 0 || ncand > kCap) return FS_OK;     // none, or so many that "long" means nothing here
  std::vector<RowLen> h((size_t)ncand);
  FS_HIP(hipMemcpy(h.data(), cand, sizeof(int2) * (size_t)ncand, hipMemcpyDeviceToHost));
  // the longest cap_rows of them, dealt out to their owners (fs_plan.h)
  std::vector<int> rows, own_first;
  std::vector<unsigned char> owner_of;
  std::vector<int64_t> lptr;
  deal_long_rows(std::move(h), cap_rows, rows, own_first, owner_of, lptr);
  const int nlong = (int)rows.size();
  const int64_t nl = lptr[(size_t)nlong];
  if (o.long_rows == 1 && !long_rows_pay(nl, A.nnz, A.ncol)) return FS_OK;
  if ((uint64_t)B * (uint64_t)nlong >= (1ull << 32)) return FS_OK;

  LongRows *L = new LongRows();
  struct Guard { LongRows *&p; bool keep = false; ~Guard() { if (!keep) free_long_rows(p); } } guard{L};
  L->nlong = nlong; L->B = B; L->bcols = bcols;
  FS_HIP(traced_malloc(&L->row, sizeof(int) * (size_t)nlong));
  FS_HIP(hipMemcpyAsync(L->row, rows.data(), sizeof(int) * (size_t)nlong, hipMemcpyHostToDevice, s));
  FS_HIP(traced_malloc(&L->ylong, sizeof(double) * (size_t)nlong));

  // ---- split the entries -------------------------------------------------------------------------------------------
  Scratch<int> row_to_long, mlen;
  Scratch<int64_t> long_ptr, start, shift;
  Scratch<unsigned> lkey, lsrc, skey, ssrc;
  Scratch<char> tmp;
  FS_HIP(row_to_long.alloc((size_t)A.nrow));
  FS_HIP(mlen.alloc((size_t)A.nrow + 1));
  FS_HIP(main_rp.alloc((size_t)A.nrow + 1));
  FS_HIP(long_ptr.alloc((size_t)nlong + 1));
  FS_HIP(hipMemsetAsync(row_to_long, 0xff, sizeof(int) * (size_t)A.nrow, s));
  FS_HIP(hipMemcpyAsync(long_ptr, lptr.data(), sizeof(int64_t) * lptr.size(), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(long_mark_kernel, dim3(grid_for(nlong)), dim3(256), 0, s, nlong, L->row, row_to_long.p);
  hipLaunchKernelGGL(main_len_kernel, dim3(grid_for((int64_t)A.nrow + 1)), dim3(256), 0, s, A.nrow, A.row_ptr, row_to_long.p, mlen.p);
  FS_HIP(hipGetLastError());
  if (int rc = device_exclusive_scan(tmp, mlen.p, main_rp.p, (size_t)A.nrow + 1, s)) return rc;
  const int64_t nm = A.nnz - nl;
  *main_nnz = nm;
  FS_HIP(main_cols.alloc((size_t)(nm > 0 ? nm : 1)));
  if (A.vals) FS_HIP(main_vals.alloc((size_t)(nm > 0 ? nm : 1)));
  FS_HIP(lkey.alloc((size_t)nl));
  FS_HIP(lsrc.alloc((size_t)nl));
  FS_HIP(skey.alloc((size_t)nl));
  FS_HIP(ssrc.alloc((size_t)nl));
  hipLaunchKernelGGL(split_entries_kernel, dim3(grid_for(A.nnz)), dim3(256), 0, s, A.nrow, A.nnz, nlong, bcols, A.row_ptr, A.cols, A.vals,
                     row_to_long.p, main_rp.p, long_ptr.p, main_cols.p, A.vals ? main_vals.p : nullptr, lkey.p, lsrc.p);
  FS_HIP(hipGetLastError());
  Scratch<char> tmp2;
  const unsigned *sorted_keys = nullptr, *sorted_src = nullptr;       // stable: CSR order inside a run
  if (int rc = device_sort_pairs(tmp2, lkey.p, skey.p, lsrc.p, ssrc.p, (size_t)nl, sort_bits((uint64_t)B * (uint64_t)nlong, 32), s,
                                 &sorted_keys, &sorted_src)) return rc;
  // the segments: (band, owner) in that order, each padded to an even count
  const int64_t nseg = (int64_t)B * kLongOwners;
  Scratch<int> d_own_first;
  Scratch<unsigned char> d_owner_of;
  FS_HIP(start.alloc((size_t)nseg + 1));
  FS_HIP(shift.alloc((size_t)nseg + 1));
  FS_HIP(d_own_first.alloc((size_t)kLongOwners + 1));
  FS_HIP(d_owner_of.alloc((size_t)nlong));
  FS_HIP(hipMemcpyAsync(d_own_first, own_first.data(), sizeof(int) * own_first.size(), hipMemcpyHostToDevice, s));
  FS_HIP(hipMemcpyAsync(d_owner_of, owner_of.data(), owner_of.size(), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(long_seg_start_kernel, dim3(grid_for(nseg + 1)), dim3(256), 0, s, B, nlong, nl, d_own_first.p, sorted_keys, start.p);
  FS_HIP(hipGetLastError());
  std::vector<int64_t> hs((size_t)nseg + 1), hp, hsh;
  std::vector<unsigned> hseg;
  FS_HIP(hipMemcpyAsync(hs.data(), start, sizeof(int64_t) * hs.size(), hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  if (!pad_long_segments(hs, B, hp, hseg, hsh)) return FS_OK;   // (a band of 4 G entries: not this path)
  L->n = hp[(size_t)B];
  FS_HIP(traced_malloc(&L->band_ptr, sizeof(int64_t) * ((size_t)B + 1)));
  FS_HIP(traced_malloc(&L->seg_ptr, sizeof(unsigned) * hseg.size()));
  FS_HIP(hipMemcpyAsync(L->band_ptr, hp.data(), sizeof(int64_t) * hp.size(), hipMemcpyHostToDevice, s));
  FS_HIP(hipMemcpyAsync(L->seg_ptr, hseg.data(), sizeof(unsigned) * hseg.size(), hipMemcpyHostToDevice, s));
  FS_HIP(hipMemcpyAsync(shift, hsh.data(), sizeof(int64_t) * hsh.size(), hipMemcpyHostToDevice, s));
  FS_HIP(traced_malloc(&L->lcol, sizeof(uint16_t) * (size_t)(L->n + 2)));
  FS_HIP(traced_malloc(&L->lrow, sizeof(uint16_t) * (size_t)(L->n + 2)));
  if (A.vals) FS_HIP(traced_malloc(&L->vals, sizeof(double) * (size_t)(L->n + 2)));
  hipLaunchKernelGGL(long_scatter_kernel, dim3(grid_for(nl)), dim3(256), 0, s, nl, nlong, bcols, sorted_keys, sorted_src, d_owner_of.p,
                     shift.p, A.cols, A.vals, L->lcol, L->lrow, L->vals);
  hipLaunchKernelGGL(long_pad_kernel, dim3(grid_for(nseg)), dim3(256), 0, s, nseg, bcols, start.p, shift.p, L->lcol, L->lrow, L->vals);
  FS_HIP(hipGetLastError());
  const int ncu = cu_count();
  const int64_t by_size = (L->n + kBinShareMin - 1) / kBinShareMin;
  L->nwg = (int)(by_size < ncu ? by_size : ncu);
  FS_HIP(traced_malloc(&L->ypart, sizeof(double) * (size_t)(L->nwg > 0 ? L->nwg : 1) * (size_t)nlong));
  FS_HIP(hipStreamSynchronize(s));
  guard.keep = true;
  *out = L;
  return FS_OK;
}

static int build_binned_impl(DeviceCsr &A, hipStream_t s, BinnedCsr *&slot, int kw)
{
  const Options &o = options();
  // short runs: the large bands and panels (fs_geometry.h kBinColsBig).  FS_BIN_BIG=0 / 1 never / always (A/B runs)
  static const int big_env = [] { const char *v = getenv("FS_BIN_BIG"); return v && *v ? atoi(v) : -1; }();
  const TwoPassGeometry g = plan_two_pass_geometry(A.nrow, A.ncol, A.nnz, kw, o.bin_rows, big_env);
  const int bcols = g.bcols, ge = g.ge;
  // ("reproducible": the copies stay in the race -- their pass 2 then adds in stream order, one wave per panel)
  if (o.binning == 0 || A.nrow == 0 || A.nnz == 0) return FS_OK;
  // (measured on 10 M x 10 M x 16: 0.75 ms against 1.06 ms tiled and 2.99 ms streaming; the two passes move
  // 20.5 bytes per entry at stream speed whatever the size of x, so the copy pays once the matrix is large
  // enough to fill the chip)
  if (o.binning == 1 && A.nnz < (4 << 20)) return FS_OK;
  const int ncu = cu_count();
  const int slots = ncu > 0 ? ncu : 256;   // pass-2 workgroups resident together (one per CU)

  // ---- virtual rows (long rows are cut exactly as for the tiled copy) ------------------------------------
  BinnedCsr *N = new BinnedCsr();
  slot = N;
  N->kw = kw;
  N->bcols = bcols;
  VirtualRows V;
  if (int rc = virtual_rows(A, s, true, kw, V, &N->vfirst, &N->yv)) return rc;
  N->split = V.split;
  N->nvrow = V.nvrow;
  const int nvrow = V.nvrow;

  // ---- plan: the panels (fs_plan.h) ------------------------------------------------------------------------
  std::vector<int> vp;
  if (int rc = V.fetch(vp, s)) return rc;
  static const double fill = [] { const char *v = getenv("FS_BIN_FILL"); return v && *v ? atof(v) / 100.0 : 0.8; }();
  static const int min_panels = [] { const char *v = getenv("FS_BIN_MIN_PANELS"); return v && *v ? atoi(v) : 1; }();
  const std::vector<int> panel_row = plan_two_pass_panels(vp, nvrow, A.nnz, g.R, slots, fill, min_panels, kw);
  const int P = (int)panel_row.size() - 1;
  const int B = (A.ncol + bcols - 1) / bcols;
  const int64_t nruns = (int64_t)P * B;
  if (nruns >= (1ll << 28)) return FS_OK;
  if (o.binning == 1 && two_pass_padding_dominates(A.nnz, nruns, ge)) return FS_OK;
  N->P = P; N->B = B; N->slots = slots;
  FS_HIP(traced_malloc(&N->panel_row, sizeof(int) * panel_row.size()));
  FS_HIP(hipMemcpyAsync(N->panel_row, panel_row.data(), sizeof(int) * panel_row.size(), hipMemcpyHostToDevice, s));

  // ---- sort the entries by (band, panel) and size the padded runs ------------------------------------------
  const size_t n = (size_t)A.nnz;
  Scratch<int> vrows, run_ptr;
  Scratch<unsigned> keys, skeys, idx_in, idx_out, g1, g2, start1, start2;
  Scratch<char> tmp, tmp2;
  FS_HIP(vrows.alloc(n));
  FS_HIP(keys.alloc(n));
  FS_HIP(skeys.alloc(n));
  FS_HIP(idx_in.alloc(n));
  FS_HIP(idx_out.alloc(n));
  FS_HIP(run_ptr.alloc((size_t)nruns + 1));
  FS_HIP(g1.alloc((size_t)nruns + 1));
  FS_HIP(g2.alloc((size_t)nruns + 1));
  FS_HIP(start1.alloc((size_t)nruns + 1));
  FS_HIP(start2.alloc((size_t)nruns + 1));
  FS_HIP(traced_malloc(&N->band_ptr, sizeof(unsigned) * ((size_t)B + 1)));
  FS_HIP(traced_malloc(&N->bin_ptr, sizeof(unsigned) * ((size_t)P + 1)));
  hipLaunchKernelGGL(bin_key_kernel, dim3(grid_for(A.nnz)), dim3(256), 0, s, nvrow, A.nnz, P, bcols, V.vrow_ptr, N->panel_row,
                     A.cols, vrows.p, keys.p);
  const unsigned *sorted_keys = nullptr, *perm = nullptr;
  if (int rc = sorted_runs(tmp, keys.p, skeys.p, idx_in.p, idx_out.p, n, nruns, run_ptr.p, s, &sorted_keys, &perm)) return rc;
  // ---- one byte per row id where the cells are dense (BinnedCsr::lrow8): the dummies that walk steps above 255, counted first ----
  Scratch<unsigned> extra, xs;
  Scratch<char> tmp3;
  bool rows8 = false;
  int64_t dummies = 0;
  if (kw == 1 && bcols == kBinCols && !(o.bin_flags & 64) && A.nnz > 0) {
    FS_HIP(extra.alloc(n + 1));
    FS_HIP(xs.alloc(n + 1));
    hipLaunchKernelGGL(bin_gap_kernel, dim3(grid_for(A.nnz + 1)), dim3(256), 0, s, A.nnz, P, sorted_keys, perm, vrows.p, run_ptr.p, extra.p);
    FS_HIP(hipGetLastError());
    if (int rc = device_exclusive_scan(tmp3, extra.p, xs.p, n + 1, s)) return rc;
    unsigned total = 0;
    if (int rc = read_back(&total, (const unsigned *)xs.p + n, s)) return rc;
    dummies = total;
    rows8 = (o.bin_flags & 128) || (double)total <= 0.01 * (double)A.nnz;
  }
  hipLaunchKernelGGL(bin_groups_kernel, dim3(grid_for(nruns + 1)), dim3(256), 0, s, B, P, ge, run_ptr.p, g1.p, g2.p,
                     rows8 ? (const unsigned *)xs.p : (const unsigned *)nullptr);
  FS_HIP(hipGetLastError());
  if (int rc = device_exclusive_scan(tmp2, g1.p, start1.p, (size_t)nruns + 1, s)) return rc;
  if (int rc = device_exclusive_scan(tmp2, g2.p, start2.p, (size_t)nruns + 1, s)) return rc;   // (the same temporary)
  hipLaunchKernelGGL(bin_ptr_kernel, dim3(grid_for((B > P ? B : P) + 1)), dim3(256), 0, s, B, P, start1.p, start2.p, N->band_ptr,
                     N->bin_ptr);
  FS_HIP(hipGetLastError());
  unsigned total_groups = 0;
  if (int rc = read_back(&total_groups, (const unsigned *)N->band_ptr + B, s)) return rc;
  const int64_t groups = total_groups;
  // every padded run adds at most ge - 1 entries: n <= nnz + 15 * nruns < 2^31 + 2^32
  if (groups >= (1ll << 28) * (int64_t)kw) return FS_OK;   // group indices are 32-bit, entry offsets 64-bit
  if (groups >= (1ll << 32) - 1) return FS_OK;
  N->n = groups * ge;
  if (o.binning == 1 && kw == 1 && two_pass_hopeless(N->n, A.vals != nullptr, B, ncu, bcols, nvrow, A.ncol, A.nnz)) return FS_OK;

  // ---- lay out both orders ------------------------------------------------------------------------------------
  const size_t np = (size_t)N->n;
  FS_HIP(traced_malloc(&N->lcol, sizeof(uint16_t) * np));
  if (rows8) {
    FS_HIP(traced_malloc(&N->lrow8, np));
    FS_HIP(traced_malloc(&N->gbase, sizeof(uint16_t) * (size_t)(groups ? groups : 1)));
    N->dummies = dummies;
  } else {
    FS_HIP(traced_malloc(&N->lrow, sizeof(uint16_t) * np));
  }
  FS_HIP(traced_malloc(&N->gdst, sizeof(unsigned) * (size_t)groups));
  FS_HIP(traced_malloc(&N->prod, sizeof(double) * np * (size_t)kw));
  if (A.vals) {
    FS_HIP(traced_malloc(&N->vals, sizeof(double) * np));
    FS_HIP(hipMemsetAsync(N->vals, 0, sizeof(double) * np, s));
  }
  FS_HIP(hipMemsetD16Async((hipDeviceptr_t)N->lcol, (unsigned short)bcols, np, s));   // padding: the zero row behind the band
  if (rows8) {
    FS_HIP(hipMemsetAsync(N->lrow8, 0, np, s));
    FS_HIP(hipMemsetAsync(N->gbase, 0, sizeof(uint16_t) * (size_t)(groups ? groups : 1), s));
    hipLaunchKernelGGL(bin_scatter8_kernel, dim3(grid_for(A.nnz)), dim3(256), 0, s, A.nnz, B, P, bcols, ge, sorted_keys, perm, vrows.p,
                       N->panel_row, A.cols, A.vals, run_ptr.p, xs.p, start1.p, start2.p, N->lcol, N->vals, N->lrow8, N->gbase);
  } else {
    FS_HIP(hipMemsetAsync(N->lrow, 0, sizeof(uint16_t) * np, s));
    hipLaunchKernelGGL(bin_scatter_kernel, dim3(grid_for(A.nnz)), dim3(256), 0, s, A.nnz, B, P, bcols, ge, sorted_keys, perm, vrows.p,
                       N->panel_row, A.cols, A.vals, run_ptr.p, start1.p, start2.p, N->lcol, N->vals, N->lrow);
  }
  hipLaunchKernelGGL(bin_gdst_kernel, dim3(grid_for(nruns)), dim3(256), 0, s, B, P, start1.p, start2.p, N->gdst);
  FS_HIP(hipGetLastError());

  // ---- pass-1 work: one persistent workgroup per CU, fewer when the shares would be tiny --------------------
  {
    const int64_t by_size = (N->n * kw + kBinShareMin - 1) / kBinShareMin;
    N->nwg1 = (int)(by_size < ncu ? by_size : ncu);
  }
  FS_HIP(hipStreamSynchronize(s));
  N->built = true;
  return FS_OK;
}

// Like the tiled copy, an optimisation: a failed build leaves the matrix on the other kernels.
int build_binned(DeviceCsr &A, hipStream_t s)
{
  LongRows *lr = nullptr;
  Scratch<int> main_rp, main_cols;
  Scratch<double> main_vals;
  int64_t main_nnz = 0;
  if (split_long_rows(A, s, &lr, main_rp, main_cols, main_vals, &main_nnz) != FS_OK) {
    free_long_rows(lr);
    (void)hipGetLastError();
  }
  int rc;
  if (lr) {
    // the copy is built from the CSR WITHOUT the long rows (a temporary of this build: the copy keeps nothing of it)
    DeviceCsr M;
    M.nrow = A.nrow; M.ncol = A.ncol; M.nnz = main_nnz;
    M.row_ptr = main_rp.p; M.cols = main_cols.p; M.vals = A.vals ? main_vals.p : nullptr; M.owns = false;
    rc = build_binned_impl(M, s, A.binned, 1);
    if (rc == FS_OK && A.binned && A.binned->built) { A.binned->lr = lr; lr = nullptr; }
    M = DeviceCsr();
  } else {
    rc = build_binned_impl(A, s, A.binned, 1);
  }
  free_long_rows(lr);
  return optional_copy(rc, A.binned, free_binned_slot);
}

// the copy that serves kw = 2 or 4 right-hand sides in one sweep (bsbm_A_mul_B2 / _B4, bcsr_A_mul_B2 / _B4, block CG):
// the north_star's "LDS-tiled dense B panel" -- a band of kBinCols / kw rows of the row-major X lives in LDS
int build_binned_k(DeviceCsr &A, int kw, hipStream_t s)
{
  if (kw != 2 && kw != 4) return FS_ERR_ARG;
  BinnedCsr *&slot = kw == 2 ? A.binned2 : A.binned4;
  (kw == 2 ? A.tried2 : A.tried4) = true;
  return optional_copy(build_binned_impl(A, s, slot, kw), slot, free_binned_slot);
}

// ---- which copy to keep ---------------------------------------------------------------------------------
// The estimates in the builders only weed out hopeless candidates.  Between the survivors (and the chunk-streaming
// kernel, which needs no copy) the choice is measured: every candidate runs the product on a zero vector -- same
// addresses and traffic as any x -- and the fastest keeps its copy; the others are released.  (Callers who need
// sums that are bit-identical from run to run set "reproducible": the LDS-staged copy leaves the race and the two-pass copy is
// timed with its ordered pass 2.)
// The L2-tiled kernel gathers from an L2-resident band of x: it has never run faster than 152 G entries per second on a matrix whose x
// does not fit L2 (config 2: 1.05 ms for 160 M entries; its gathers alone are bound at 205 G/s, profiles/r04_probe_gather.jsonl), where the
// two-pass pair streams 200 G valued / 280 G pattern entries per second.  So on a large matrix whose two-pass copy, just built, already
// beats that rate, the L2-tiled copy is not built at all (config 2: 34 + 6 of 115 ms per matrix, and its transient HBM), and the
// streaming kernel -- three to four times slower there -- is timed once instead of five times.  Auto mode only.
constexpr double kTiledBestEntriesPerMs = 152e6;          // valued; pattern-only: 200e6 (config 2's pattern: 0.817 ms = 196 G/s, profiles/r03_cg_kernel_stats.csv)

template <typename F>
static int time_product(F launch, hipStream_t s, hipEvent_t e0, hipEvent_t e1, float *median, int reps = 5)
{
  float t[5] = {1e30f, 1e30f, 1e30f, 1e30f, 1e30f};
  for (int rep = -1; rep < reps; ++rep) {   // run -1 warms the instruction cache and the TLB
    FS_HIP(hipEventRecord(e0, s));
    if (int rc = launch()) return rc;
    FS_HIP(hipEventRecord(e1, s));
    FS_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    FS_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (rep >= 0) t[rep] = ms;
  }
  std::sort(t, t + reps);
  *median = t[reps / 2];                   // the tiled kernel's fastest run is not typical of it; its median is
  return FS_OK;
}

int two_pass_clear_win(DeviceCsr &A, hipStream_t s, bool *win)
{
  *win = false;
  const Options &o = options();
  if (!(A.binned && A.binned->built) || o.binning != 1 || o.tiling != 1 || A.nnz < (32ll << 20) || 8.0 * (double)A.ncol <= (double)(4 << 20)) return FS_OK;
  Scratch<double> x, y;
  if (x.alloc((size_t)A.ncol) != hipSuccess || y.alloc((size_t)A.nrow) != hipSuccess) { (void)hipGetLastError(); return FS_OK; }
  FS_HIP(hipMemsetAsync(x, 0, sizeof(double) * (size_t)A.ncol, s));
  hipEvent_t e0, e1;
  FS_HIP(hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return FS_OK; }
  float t = 1e30f;
  const int rc = time_product([&] { return launch_spmv_binned(A, y, x, s); }, s, e0, e1, &t, 2);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc != FS_OK) return rc;
  *win = (double)t <= (double)A.nnz / (A.vals ? kTiledBestEntriesPerMs : 200e6);
  return FS_OK;
}

int choose_copy(DeviceCsr &A, hipStream_t s)
{
  BuildClock clock(s);
  const Options &o = options();
  const bool hb = A.binned && A.binned->built, ht = A.tiled && A.tiled->built, hx = A.tiledx && A.tiledx->built;
  if (!hb && !ht && !hx) return FS_OK;
  if (o.tiling == 2 || o.binning == 2 || o.ldsx == 2) {   // the caller chose: keep what was asked for, nothing else
    if (o.binning != 2) free_binned_slot(A.binned);
    if (o.ldsx != 2) free_tiled_slot(A.tiledx);
    if (o.tiling != 2) free_tiled_slot(A.tiled);
    return FS_OK;
  }
  Scratch<double> x, y;
  if (x.alloc((size_t)A.ncol) != hipSuccess || y.alloc((size_t)A.nrow) != hipSuccess) {
    (void)hipGetLastError();
    return FS_OK;                                                       // no room to measure: keep the estimate's order
  }
  FS_HIP(hipMemsetAsync(x, 0, sizeof(double) * (size_t)A.ncol, s));
  hipEvent_t e0, e1;
  FS_HIP(hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return FS_OK; }
  float t_stream = 1e30f, t_tiled = 1e30f, t_bin = 1e30f, t_ldsx = 1e30f;
  // (a lone LDS-staged copy with dense tiles -- build_schedule did not build its rivals -- is 8 to 15 times faster than the
  // streaming kernel: one timed run of that one is enough to say so, five cost 25-50 ms of a 230 ms build on config 3)
  const bool lone_ldsx = hx && !hb && !ht && A.tiledx->entries_per_tile >= kLdsxClearWin;
  int rc = time_product([&] { return launch_spmv(A, y, x, s, true); }, s, e0, e1, &t_stream, (lone_ldsx || A.two_pass_clear_win) ? 1 : 5);
  if (rc == FS_OK && ht) rc = time_product([&] { return launch_spmv_tiled(A, *A.tiled, y, x, s); }, s, e0, e1, &t_tiled);
  if (rc == FS_OK && hx) rc = time_product([&] { return launch_spmv_tiled(A, *A.tiledx, y, x, s); }, s, e0, e1, &t_ldsx);
  if (rc == FS_OK && hb) rc = time_product([&] { return launch_spmv_binned(A, y, x, s); }, s, e0, e1, &t_bin);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc != FS_OK) return rc;
  A.build_ms[6] = clock.lap();
  A.candidate_ms[0] = t_stream;
  A.candidate_ms[1] = ht ? t_tiled : 0.f;
  A.candidate_ms[2] = hx ? t_ldsx : 0.f;
  A.candidate_ms[3] = hb ? t_bin : 0.f;
  float best = t_stream;
  if (t_tiled < best) best = t_tiled;
  if (t_ldsx < best) best = t_ldsx;
  if (t_bin < best) best = t_bin;
  // Candidates within 5 % of the fastest count as equal (box-to-box and run-to-run differences are of that size) and a
  // fixed priority decides between them -- two-pass, LDS-staged, L2-tiled, streaming -- so that the same matrix gets the
  // same kernel (and the same summation order) on every run and for A as for A' unless one kernel really is faster.
  const float tie = best * 1.05f;
  const int keep = (hb && t_bin <= tie) ? 3 : (hx && t_ldsx <= tie) ? 2 : (ht && t_tiled <= tie) ? 1 : 0;
  if (keep != 3) free_binned_slot(A.binned);
  if (keep != 2) free_tiled_slot(A.tiledx);
  if (keep != 1) free_tiled_slot(A.tiled);
  A.build_ms[7] = clock.lap();
  return FS_OK;
}

}  // namespace fs
