// fs_dist.hip -- the row-sharded products on the GPUs of one node, inside the C-ABI (include/fastsparse_hip.h, "several
// GPUs"): one process, N devices, rows cut by non-zeros, the input vector replicated, the output all-gathered over RCCL
// (xGMI) WHILE the product still runs.
//
// This is the north_star's "host C dispatching through a thin C-ABI ... rows range-partitioned across the 8 GPUs of one
// node with y gathered via RCCL" for a plain C caller: EVERY product entry point of sparse.h / dsparse.h / csr.h / cbcsr.h / cg.h
// takes this path when FASTSPARSE_NGPU > 1 (fs_dropin.hip, "several GPUs").  The Python bench uses one process per GPU and torch.distributed over the
// same RCCL (libfastsparse_amd/dist.py); both shard the same way.
//
// Both directions are "rows + all-gather" ("prefer holding CSR' row-sharded too"):
//   y = A x   rank r owns rows [bounds[r], bounds[r+1]) of A (equal non-zeros), x replicated;
//   z = A' u  rank r owns rows of A' (= columns of A, again cut by non-zeros), u replicated -- and u IS y after a product, so
//             A then A' needs no copy.  The shards of A' are built from host arrays (fs_dist_matrix_build_transpose) or, with no
//             whole-matrix host array anywhere, from the device-resident shards of A (fs_dist_matrix_build_transpose_device).
// A matrix comes from ONE host CSR (fs_dist_csr_create: int row_ptr, < 2^31 entries in total) or from per-rank shards
// (fs_dist_csr_create_from_shards: every shard < 2^31 entries, the total is 64-bit -- BASELINE config 5 only exists this way).
//
// ONE PLAN: the layout of an exchange -- which window of a rank's local output every all-gather sends, where rank r's rows land in the
// padded buffer, the tables of the unpack, the buffer sizes -- is fs::plan_exchange (fs_dist_plan.h: plain C++, tested without a
// GPU) for every k; the cuts it starts from come from the kernels (fs_spmv_part_rows, fs_spmm_part_rows).  A DistSide owns the
// k = 1 plan of its side, KWork one plan per side for the handle's current k > 1.
// ONE ENGINE: run_product runs a product for any k, run_gather the whole-shard exchange, on a small view (Exchange).  The local
// product runs in parts (fs_spmv_part / fs_spmm_part) on the rank's compute stream; behind every part an event lets the rank's
// COMMUNICATION stream all-gather the rows that part finished -- one ncclAllGather per part on a padded buffer (counts differ
// between ranks) -- while the next part computes; one fs_copy_segments launch per rank unpacks the padded buffer into the full
// vector at the end.  No n^2 broadcasts, no host round trip.  Every step is "for every rank do f(r)" (each_rank): on the calling
// thread, or on one issuing thread per rank (RankWorkers).  What differs between the modes is behaviour, each kept in one place:
//   1  whole-shard mode (ONE all-gather behind the finished local product: no send window reaches into rows still being written):
//      k = 1 when conservative || np == 1, launched as all np calls of fs_spmv_part; k > 1 when conservative || np <= 1 || !real,
//      launched as ONE fs_spmm (dist_product);
//   2  replan_if_moved runs for k = 1 products only; ensure_k rebuilds the k-column plans on any option-epoch change (dist_product);
//   3  RCCL from the calling thread: ncclGroupStart, one ncclAllGather per rank in rank order, ncclGroupEnd; issuing threads: each
//      its own call, no group; virtual ranks: per destination, wait for every rank's event, then copy (exchange_equal);
//   4  a failed exchange, calling thread: conservative = true; with RCCL the communicators are aborted (abort_communicators: no
//      second collective on a half-issued group) and the context returns errors from then on; on virtual ranks the remaining parts
//      run, then dist_sync, then one whole-shard gather.  Issuing threads: the error is returned, no fallback.  FS_DIST_FAIL_PART is
//      honoured only when the calling thread issues (run_product);
//   5  k > 1 under FS_DIST_THREADS=1 is issued by the calling thread: an inherited asymmetry, not a decision (dist_product);
//   6  the broken check first, then ++g_products, once per product (dist_product);
//   7  events: whole-shard mode uses ev[r][0], overlapped mode ev[r][p]; done[r] follows the unpack and the compute stream waits
//      for it (run_gather, run_product).
// The CONSERVATIVE mode is FS_DIST_PARTS=1, or what a context falls to after a failed exchange (4).
// The caller's vectors may live in host memory or in the HBM of any device (vec_in / vec_out): a vector in HBM is read in place by
// the ranks of its device, travels device to device to the others, and an output in HBM is written by the unpack launch itself.
//
// RCCL is loaded with dlopen when the first context with more than one distinct device is created, so that
// single-GPU users never load it and a process that already holds a copy (PyTorch ships one) shares it.
// A context whose device list names the same device more than once ("virtual ranks": RCCL refuses duplicates)
// exchanges the parts with device-to-device copies instead; that form exists so that the sharding, the parts and the
// padded layout can be exercised on a one-GPU machine (tests/test_gpu_parity.py) and is not a substitute for RCCL on
// real devices.  UNVERIFIED ON HARDWARE: RCCL with MORE THAN ONE rank has not run anywhere yet (no multi-GPU machine was
// available to the builder); FS_DIST_FORCE_RCCL=1 takes a one-device context through the same group calls.
#include <dlfcn.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include <rccl/rccl.h>

#include "csr.h"
#include "fs_common.h"
#include "fs_dist_plan.h"

namespace {

struct Rccl {
  void *lib = nullptr;
  decltype(&ncclCommInitAll) CommInitAll = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclCommAbort) CommAbort = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  bool ok = false;
};

Rccl &rccl()
{
  static Rccl r = [] {
    Rccl q;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      q.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (q.lib) break;
    }
    if (!q.lib) return q;
#define FS_SYM(f) q.f = reinterpret_cast<decltype(q.f)>(dlsym(q.lib, "nccl" #f))
    FS_SYM(CommInitAll); FS_SYM(CommDestroy); FS_SYM(CommAbort); FS_SYM(GroupStart); FS_SYM(GroupEnd); FS_SYM(AllGather); FS_SYM(GetErrorString);
#undef FS_SYM
    q.ok = q.CommInitAll && q.CommDestroy && q.GroupStart && q.GroupEnd && q.AllGather && q.GetErrorString;
    return q;
  }();
  return r;
}

int nccl_fail(ncclResult_t e, const char *what)
{
  fs::set_error(std::string("RCCL error in ") + what + ": " + (rccl().GetErrorString ? rccl().GetErrorString(e) : "?"));
  return FS_ERR_HIP;
}

// the calling thread gets its current device back however the function leaves
struct DeviceGuard {
  int dev = -1;
  DeviceGuard() { if (hipGetDevice(&dev) != hipSuccess) dev = -1; }
  ~DeviceGuard() { if (dev >= 0) (void)hipSetDevice(dev); }
};

// FS_DIST_FAIL_PART (tests): the exchange of part p fails, once per process -- whichever product gets there first
bool take_injection(int p);
std::atomic<long> g_products{0};     // sharded products launched by this process (fs_debug_dist_products: the tests' proof of the path taken)

int env_parts()
{
  static const int v = [] {
    const char *e = getenv("FS_DIST_PARTS");
    const int p = e && *e ? atoi(e) : 4;
    return p < 1 ? 1 : (p > 16 ? 16 : p);
  }();
  return v;
}

// FS_DIST_FAIL_PART=p (tests only): the all-gather of part p of the next overlapped product reports an error once, which takes
// the context to the conservative mode -- the only way to walk that path without a broken fabric
int env_fail_part()
{
  static const int v = [] { const char *e = getenv("FS_DIST_FAIL_PART"); return e && *e ? atoi(e) : -1; }();
  return v;
}

bool take_injection(int p)
{
  static std::atomic<bool> injected{false};
  return env_fail_part() == p && !injected.exchange(true);
}

}  // namespace

// One ISSUING thread per rank (FS_DIST_THREADS=1; experimental, off by default).  One host thread pays about 50 us per rank and
// product for the launches, events and exchange calls of the ranks one after the other (profiles/r05_dist_host_overhead.txt): at
// N = 8 the one-process path is issue-bound for products below ~0.5 ms.  With this switch every rank's calls come from a thread of
// its own -- its device current once and for all -- and a product is a few rounds of "every rank does its piece, then all meet".
// With RCCL each thread issues ITS communicator's ncclAllGather (no group: the many-threads-one-device-each form of the API).
// UNVERIFIED on more than one GPU, like the rest of this file; libfastsparse_amd/native_dist_bench.py times it beside the default.
struct RankWorkers {
  int n = 0;
  std::vector<std::thread> th;
  std::mutex m;
  std::condition_variable go, done;
  std::function<int(int)> job;
  unsigned long gen = 0;
  int pending = 0, fixed_order = 0;
  bool stop = false;
  std::vector<int> rc;
  std::vector<std::string> err;

  void start(const std::vector<int> &dev)
  {
    n = (int)dev.size();
    rc.assign((size_t)n, 0);
    err.assign((size_t)n, std::string());
    for (int r = 0; r < n; ++r)
      th.emplace_back([this, r, d = dev[(size_t)r]] {
        (void)hipSetDevice(d);
        unsigned long seen = 0;
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
          go.wait(lk, [&] { return stop || gen != seen; });
          if (stop) return;
          seen = gen;
          const std::function<int(int)> f = job;
          const int fo = fixed_order;
          lk.unlock();
          fs::tl_fixed_order = fo;              // the caller's solver scope (thread-local there) holds for its ranks' launches too
          const int code = f(r);
          const std::string why = code ? fs_last_error() : "";
          fs::tl_fixed_order = 0;
          lk.lock();
          rc[(size_t)r] = code;
          err[(size_t)r] = why;
          if (--pending == 0) done.notify_one();
        }
      });
  }
  // f(r) on every rank's thread; returns when all are back: the first error (its message becomes the caller's), or FS_OK
  int run(const std::function<int(int)> &f)
  {
    std::unique_lock<std::mutex> lk(m);
    job = f;
    fixed_order = fs::tl_fixed_order;
    pending = n;
    ++gen;
    go.notify_all();
    done.wait(lk, [&] { return pending == 0; });
    for (int r = 0; r < n; ++r)
      if (rc[(size_t)r]) { fs::set_error(err[(size_t)r]); return rc[(size_t)r]; }
    return FS_OK;
  }
  ~RankWorkers()
  {
    {
      std::lock_guard<std::mutex> lk(m);
      stop = true;
    }
    go.notify_all();
    for (std::thread &t : th) t.join();
  }
};

struct fs_dist_s {
  int n = 0;
  std::vector<int> dev;               // device of every rank
  std::vector<hipStream_t> stream;    // compute stream per rank, on its device
  std::vector<hipStream_t> comm_stream;  // communication stream per rank
  bool use_rccl = false;
  bool conservative = false;          // one whole-shard all-gather behind the product (FS_DIST_PARTS=1, or after an error)
  bool broken = false;                // an RCCL call failed: the communicators were aborted, every later product is an error return
  std::unique_ptr<RankWorkers> workers;   // FS_DIST_THREADS=1: one issuing thread per rank (else null: the calling thread issues)
  std::vector<ncclComm_t> comm;
  std::mutex lock;                    // the streams and communicators serve one product at a time (a communicator must not be
                                      // used from two host threads at once): taken behind the matrix's own lock
};

// one direction of a distributed matrix: row shards of M (A, or A'), input replicated, output gathered
struct DistSide {
  int nrow = 0, ncol = 0;             // of M
  std::vector<int> bounds;            // rank r owns rows [bounds[r], bounds[r + 1]) of M
  std::vector<int64_t> shard_nnz;
  std::vector<fs_matrix_t> shard;
  fs::ExchangePlan plan;              // of the single-vector product (k = 1): cuts from fs_spmv_part_rows
  // per rank, on its device: the shard's rows of the output (room for a padded window behind the last row), the padded
  // receive buffer, the table of the unpack launches (plan.table), one event per part
  std::vector<double *> local, pad;
  std::vector<int64_t *> table;
  std::vector<std::vector<hipEvent_t>> ev;   // [rank][part]; the k-column products of the side use them too
  std::vector<hipEvent_t> done;              // [rank]: the unpack on the communication stream
  bool built = false;
  unsigned epoch = 0;                 // fs::option_epoch() when the cuts were last checked against the kernels (replan_if_moved)
};

// Device buffers of one work space, per rank: each allocated with the rank's device current and freed there.  `ready` only after
// every allocation of a fill succeeded: a failure leaves it false, and the next call frees what exists and starts over.
struct RankBuffers {
  std::vector<std::vector<void *>> held;   // [rank], in the order of allocation
  bool ready = false;

  // `count` elements at v[r], on the current device (rank r's)
  template <typename T>
  int get(int r, std::vector<T *> &v, size_t count)
  {
    v.resize(held.size(), nullptr);
    FS_HIP(hipMalloc(&v[(size_t)r], sizeof(T) * count));
    held[(size_t)r].push_back(v[(size_t)r]);
    return FS_OK;
  }
  // per_rank(r) makes rank r's allocations (and whatever fills them), its device current
  int fill(fs_dist_t D, const std::function<int(int)> &per_rank)
  {
    held.assign((size_t)D->n, std::vector<void *>());
    for (int r = 0; r < D->n; ++r) {
      FS_HIP(hipSetDevice(D->dev[r]));
      if (int rc = per_rank(r)) return rc;
    }
    ready = true;
    return FS_OK;
  }
  void release(fs_dist_t D)
  {
    for (size_t r = 0; r < held.size(); ++r) {
      (void)hipSetDevice(D->dev[r]);
      for (void *p : held[r]) (void)hipFree(p);
    }
    held.clear();
    ready = false;
  }
};

struct CgWork {                       // vectors of fs_dist_cg / fs_dist_pcg, kept on the handle between solves
  int F = 0;
  RankBuffers mem;
  // red: two send slots of kCgSendDoubles and the finished sums behind them; redall: every rank's slot, gathered
  std::vector<double *> sol, r, b, p, q, dinv, part, red, redall, st;
};
constexpr int kCgSendDoubles = 2;     // sums one exchange carries per rank: {b.b, r.r} and {r.r, r.z} of fs_dist_pcg

// fs_dist_pcgn's own vectors for k columns (whole panels on every rank), kept like CgWork; P, T, Q are the product vectors of the
// handle (x / y / z, or KWork's for k > 1)
// fs_dist_pcgn_lambdas on slices keeps rank r's rows of A' of X, R, B, Q (q) and of s / dinv instead: n_r k doubles each; send: two
// send slots of kPcgnSendDoubles and all: every rank's slot, gathered.  The slice of P is the transposed side's local buffer
struct PnWork {
  int F = 0, k = 0;
  bool slices = false;
  RankBuffers mem;
  std::vector<double *> sol, r, b, dinv, part, cs, st;
  std::vector<double *> q, send, all;
};

// A ladder solver's own vectors, kept like CgWork: the x_i (X, room for m of them) and the directions P_i of the shifts with
// sigma != 0 (P, room for nslots), whole or the rank's slice, ld doubles apart (ld even); sc: the solver's scalars.  The handle
// keeps one for each ladder solver, so interleaved solves of the two leave each other's vectors alone:
//   ms  fs_dist_mscg's: vectors of F doubles; sc is the per-shift array.  r, b, p, q and the sums are CgWork's
//   mn  fs_dist_mscgn's: F x k panels or the rank's rows of A' of them; sc holds the finished sums the scalar steps read, then
//       cst / ms / sl: every column's st[] and ms[] and the per-shift list -- one allocation, cleared at the start of a solve.
//       R, B, Q, the partials, the send slots and st are PnWork's
struct LadderWork {
  int F = 0, m = 0, nslots = 0;
  long long ld = 0;
  RankBuffers mem;
  std::vector<double *> X, P, sc;
};
constexpr size_t kMnCstDoubles = (size_t)FS_PCGN_MAX_RHS * fs::kCgStateDoubles;
constexpr size_t kMnScalarDoubles = (size_t)fs::kPcgnSendDoubles + kMnCstDoubles + fs::kMscgnStateDoubles + fs::kMscgnListDoubles;

// k row-major columns on the sharded matrix (fs_dist_spmm, fs_dist_cg2): the replicated X / Y / Z, the shards' local outputs, the
// padded receive buffer (one, for both sides), the unpack tables and the work vectors of the block solver, per rank; one plan per
// side, its cuts from fs_spmm_part_rows (the one-sweep plan of k = 2, 4 is cut like the single-vector pair)
struct KWork {
  int k = 0;
  bool with_t = false;
  unsigned epoch = 0;                   // fs::option_epoch() when the parts were planned
  RankBuffers mem;                      // ready: every prepare and allocation of ensure_k succeeded
  fs::ExchangePlan pa, pt;
  std::vector<double *> x, y, z, la, lt, pad;
  std::vector<int64_t *> tab;           // [rank]: pa.table, then pt.table
  std::vector<double *> sol, r, b, part, red, st;
};

struct fs_dist_matrix_s {
  fs_dist_t D = nullptr;
  int nrow = 0, ncol = 0;
  int64_t nnz = 0;
  // A (always) and A' (fs_dist_matrix_build_transpose[_device], or ANOTHER matrix's A side: fs_dist_matrix_pair).  The sides are
  // shared, not copied, between a pair and the matrices it was made from; the last owner frees the shards (side_owner).
  std::shared_ptr<DistSide> pa, pt;
  DistSide &a, &t;
  fs_dist_matrix_s(std::shared_ptr<DistSide> A, std::shared_ptr<DistSide> T) : pa(std::move(A)), pt(std::move(T)), a(*pa), t(*pt) {}
  // per rank: the whole x (ncol), y (nrow) and z (ncol) on its device.  u of z = A' u is y.
  std::vector<double *> x, y, z;
  // host copies of the CSR are NOT kept
  double *pin = nullptr;              // pinned staging of host vectors
  size_t pin_doubles = 0;
  CgWork cg;
  PnWork pn;
  LadderWork ms, mn;
  KWork kw;
  std::mutex lock;                    // products on one matrix are serialised (x, y, z and the part buffers are per matrix)
};

namespace {

void free_plan(fs_dist_t D, DistSide &S);

void free_side(fs_dist_t D, DistSide &S)
{
  free_plan(D, S);
  for (size_t r = 0; r < S.shard.size(); ++r) {
    (void)hipSetDevice(D->dev[r]);
    if (S.shard[r]) fs_matrix_destroy(S.shard[r]);
  }
  S = DistSide();
}

// a work space of the handle (CgWork, PnWork, LadderWork, KWork) back to its empty state
template <typename Work>
void free_work(fs_dist_t D, Work &W) { W.mem.release(D); W = Work(); }

// row cuts with (almost) equal numbers of non-zeros: bounds[r] = first row whose row_ptr is >= r/n of nnz -- the cut
// libfastsparse_amd/dist.py nnz_balanced_partition makes, essential for power-law matrices (BASELINE config 5)
template <typename RP>
void nnz_cut(std::vector<int> &bounds, int n, int nrow, const RP *row_ptr)
{
  const int64_t nnz = (int64_t)row_ptr[nrow];
  bounds.assign((size_t)n + 1, 0);
  for (int r = 1; r < n; ++r) {
    const int64_t target = nnz * r / n;
    int b = (int)(std::lower_bound(row_ptr, row_ptr + nrow + 1, target, [](RP a, int64_t t) { return (int64_t)a < t; }) - row_ptr);
    if (b > nrow) b = nrow;
    bounds[(size_t)r] = b < bounds[(size_t)r - 1] ? bounds[(size_t)r - 1] : b;
  }
  bounds[(size_t)n] = nrow;
}

int dist_sync(fs_dist_t D);

// the buffers, table and events of the side's k = 1 plan (the plan itself stays: replan_if_moved reads its part count)
void free_plan(fs_dist_t D, DistSide &S)
{
  for (size_t r = 0; r < S.local.size(); ++r) {
    (void)hipSetDevice(D->dev[r]);
    if (S.local[r]) (void)hipFree(S.local[r]);
    if (r < S.pad.size() && S.pad[r]) (void)hipFree(S.pad[r]);
    if (r < S.table.size() && S.table[r]) (void)hipFree(S.table[r]);
    if (r < S.ev.size()) for (hipEvent_t e : S.ev[r]) if (e) (void)hipEventDestroy(e);
    if (r < S.done.size() && S.done[r]) (void)hipEventDestroy(S.done[r]);
  }
  S.local.clear(); S.pad.clear(); S.table.clear(); S.ev.clear(); S.done.clear();
}

// The exchange plan of the side's product with k columns in np parts: the cuts come from the kernels that will run (device-handle
// calls: fs_spmv_part_rows, fs_spmm_part_rows on the prepared k-column copy), everything else is fs::plan_exchange
int side_plan(fs_dist_t D, const DistSide &S, int k, int np, fs::ExchangePlan &P)
{
  std::vector<std::vector<int>> cut((size_t)D->n, std::vector<int>((size_t)np + 1, 0));
  for (int r = 0; r < D->n; ++r) {
    if (S.bounds[(size_t)r + 1] == S.bounds[(size_t)r]) continue;
    FS_HIP(hipSetDevice(D->dev[r]));
    if (int rc = k == 1 ? fs_spmv_part_rows(S.shard[(size_t)r], 0, np, cut[(size_t)r].data())
                        : fs_spmm_part_rows(S.shard[(size_t)r], 0, k, np, cut[(size_t)r].data())) return rc;
  }
  P = fs::plan_exchange(D->n, k, S.bounds, std::move(cut));
  return FS_OK;
}

// after the shards exist: the k = 1 plan of the side, its buffers, table and events
int plan_side(fs_dist_t D, DistSide &S, int nparts)
{
  const int n = D->n;
  if (int rc = side_plan(D, S, 1, nparts, S.plan)) return rc;
  const fs::ExchangePlan &P = S.plan;
  S.local.assign((size_t)n, nullptr);
  S.pad.assign((size_t)n, nullptr);
  S.table.assign((size_t)n, nullptr);
  S.ev.assign((size_t)n, std::vector<hipEvent_t>());
  S.done.assign((size_t)n, nullptr);
  for (int r = 0; r < n; ++r) {
    FS_HIP(hipSetDevice(D->dev[r]));
    FS_HIP(hipMalloc(&S.local[(size_t)r], sizeof(double) * (size_t)P.local_rows));
    FS_HIP(hipMalloc(&S.pad[(size_t)r], sizeof(double) * (size_t)(P.pad_rows + 1)));
    FS_HIP(hipMalloc(&S.table[(size_t)r], sizeof(int64_t) * (P.table.size() + 1)));
    if (!P.table.empty()) FS_HIP(hipMemcpy(S.table[(size_t)r], P.table.data(), sizeof(int64_t) * P.table.size(), hipMemcpyHostToDevice));
    for (int p = 0; p < nparts; ++p) {
      hipEvent_t e = nullptr;
      FS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      S.ev[(size_t)r].push_back(e);
    }
    FS_HIP(hipEventCreateWithFlags(&S.done[(size_t)r], hipEventDisableTiming));
  }
  S.built = true;
  S.epoch = fs::option_epoch();
  return FS_OK;
}

int context_usable(fs_dist_t D)
{
  if (!D->broken) return FS_OK;
  fs::set_error("fs_dist: this context is unusable after an RCCL error (its communicators were aborted)");
  return FS_ERR_HIP;
}

// An RCCL call that failed (its error is the current one, `rc` its code) may have launched the collective on some ranks only:
// nothing issued on these communicators can be relied on to finish, and a new collective on them is undefined.  Abort them (that
// also ends what is in flight) and leave the context unusable: this product and every later one return the error.
// (no second collective on a failed group.)
int abort_communicators(fs_dist_t D, int rc)
{
  const std::string why = fs_last_error();
  for (ncclComm_t &c : D->comm)
    if (c) { if (rccl().CommAbort) (void)rccl().CommAbort(c); c = nullptr; }
  D->broken = true;
  fs::set_error(why + "; the RCCL communicators were aborted: create a new context");
  return rc;
}

// for every rank r do f(r): on the calling thread, rank after rank with the rank's device current, or (`threads`) on the ranks'
// issuing threads, all at once -- returns when every rank is back
int each_rank(fs_dist_t D, bool threads, const std::function<int(int)> &f)
{
  if (threads) return D->workers->run(f);
  for (int r = 0; r < D->n; ++r) {
    FS_HIP(hipSetDevice(D->dev[r]));
    if (int rc = f(r)) return rc;
  }
  return FS_OK;
}

// `count` doubles from every rank's send[r] to every rank's recv[d] + r * count, on the streams `st` (ordered behind the
// events ready[r], one per rank, recorded on whatever stream produced send[r]).
//   RCCL, calling thread    ncclGroupStart, one ncclAllGather per rank in rank order, ncclGroupEnd;
//   RCCL, issuing threads   every rank's thread makes ITS communicator's call, no group (many threads, one device each);
//   virtual ranks           per destination d (either way of issuing): wait for every rank's event, then copy -- the same layout.
// An RCCL call that returned an error aborts the communicators: nothing of this exchange can be relied on.
// inject_failure (tests, calling thread only): the exchange fails half-issued.
int exchange_equal(fs_dist_t D, const std::vector<const double *> &send, const std::vector<double *> &recv, size_t count,
                   const std::vector<hipStream_t> &st, const std::vector<hipEvent_t> &ready, bool threads = false, bool inject_failure = false)
{
  const int n = D->n;
  if (int rc = context_usable(D)) return rc;
  if (!count) return FS_OK;
  if (D->use_rccl && threads) {
    std::vector<ncclResult_t> res((size_t)n, ncclSuccess);
    (void)D->workers->run([&](int r) -> int {
      res[(size_t)r] = rccl().AllGather(send[(size_t)r], recv[(size_t)r], count, ncclDouble, D->comm[(size_t)r], st[(size_t)r]);
      return FS_OK;
    });
    for (int r = 0; r < n; ++r)
      if (res[(size_t)r] != ncclSuccess) return abort_communicators(D, nccl_fail(res[(size_t)r], "ncclAllGather (issuing threads)"));
    return FS_OK;
  }
  if (D->use_rccl) {
    // every rank's call in one group; an error inside the group still closes it
    ncclResult_t first = rccl().GroupStart();
    if (first != ncclSuccess) return nccl_fail(first, "ncclGroupStart");
    for (int r = 0; r < n && first == ncclSuccess; ++r) {
      if (inject_failure && r == (n > 1 ? 1 : 0)) { first = ncclInternalError; break; }   // (tests: rank 0's call is already in the group)
      first = rccl().AllGather(send[(size_t)r], recv[(size_t)r], count, ncclDouble, D->comm[(size_t)r], st[(size_t)r]);
    }
    const ncclResult_t end = rccl().GroupEnd();
    if (first == ncclSuccess && end == ncclSuccess) return FS_OK;
    return abort_communicators(D, first != ncclSuccess ? nccl_fail(first, "ncclAllGather") : nccl_fail(end, "ncclGroupEnd"));
  }
  return each_rank(D, threads, [&](int d) -> int {
    // (tests: the failure comes with the first destination's copies already enqueued -- a half-issued exchange)
    if (inject_failure && d == (n > 1 ? 1 : 0)) { fs::set_error("injected failure of an exchange (FS_DIST_FAIL_PART)"); return FS_ERR_HIP; }
    for (int r = 0; r < n; ++r) {
      FS_HIP(hipStreamWaitEvent(st[(size_t)d], ready[(size_t)r], 0));
      FS_HIP(hipMemcpyAsync(recv[(size_t)d] + (int64_t)r * (int64_t)count, send[(size_t)r], sizeof(double) * count, hipMemcpyDeviceToDevice,
                            st[(size_t)d]));
    }
    return FS_OK;
  });
}

// the cuts belong to the kernel the options select NOW (strict_order / reproducible / spmv_kernel set since the plan was
// made move the product to another kernel, which finishes its rows elsewhere): plan again when they moved
int replan_if_moved(fs_dist_t D, DistSide &S)
{
  const int n = D->n, np = S.plan.np;
  const unsigned epoch = fs::option_epoch();
  if (S.epoch == epoch) return FS_OK;     // no option was set since the last check: the products run on the same kernels
  bool same = true;
  std::vector<int> now((size_t)np + 1);
  for (int r = 0; same && r < n; ++r) {
    if (S.bounds[(size_t)r + 1] == S.bounds[(size_t)r]) continue;
    FS_HIP(hipSetDevice(D->dev[r]));
    if (int rc = fs_spmv_part_rows(S.shard[(size_t)r], 0, np, now.data())) return rc;
    same = now == S.plan.cut[(size_t)r];
  }
  if (!same) {
    if (int rc = dist_sync(D)) return rc;
    free_plan(D, S);
    if (int rc = plan_side(D, S, np)) return rc;
  }
  S.epoch = epoch;
  return FS_OK;
}

// What the engine below works on: one side's product with k columns -- its plan, the per-rank buffers the plan was sized for,
// the side's events, and how a rank's local product is launched (on its compute stream, the rank's device current).
struct Exchange {
  const fs::ExchangePlan &P;
  int k;
  const std::vector<double *> &local, &pad;
  const std::vector<int64_t *> &table;             // [rank]: the device copy of P.table starts at table[r] + table_at
  size_t table_at;
  const std::vector<std::vector<hipEvent_t>> &ev;  // [rank][part]
  const std::vector<hipEvent_t> &done;             // [rank]
  std::function<int(int, int)> part;               // (r, p): part p of rank r's local product
  std::function<int(int)> whole;                   // (r): the whole local product of rank r
};

// The whole-shard all-gather: rank r's rows from src[r] (room for max_rows * k doubles) into out[d] on every rank d -- after
// launch(r), the rank's whole local product, where one is given.  Runs on the communication streams behind the compute streams'
// work so far (events ev[r][0]); the unpack is followed by done[r], which the compute stream waits for.
int run_gather(fs_dist_t D, const Exchange &X, const std::vector<double *> &src, const std::vector<double *> &out, bool threads,
               const std::function<int(int)> *launch = nullptr)
{
  const fs::ExchangePlan &P = X.P;
  const int n = D->n;
  std::vector<const double *> send((size_t)n);
  std::vector<hipEvent_t> ready((size_t)n);
  if (int rc = each_rank(D, threads, [&](int r) -> int {
        if (launch)
          if (int rc2 = (*launch)(r)) return rc2;
        FS_HIP(hipEventRecord(X.ev[(size_t)r][0], D->stream[r]));
        FS_HIP(hipStreamWaitEvent(D->comm_stream[r], X.ev[(size_t)r][0], 0));
        send[(size_t)r] = src[(size_t)r];
        ready[(size_t)r] = X.ev[(size_t)r][0];
        return FS_OK;
      })) return rc;
  if (int rc = exchange_equal(D, send, X.pad, (size_t)P.window_rows * (size_t)X.k, D->comm_stream, ready, threads)) return rc;
  return each_rank(D, threads, [&](int r) -> int {
    if (int rc = fs_copy_segments(P.nseg1, P.whole_shard_table(X.table[(size_t)r] + X.table_at), P.window_rows * X.k, X.pad[(size_t)r],
                                  out[(size_t)r], D->comm_stream[r])) return rc;
    FS_HIP(hipEventRecord(X.done[(size_t)r], D->comm_stream[r]));
    FS_HIP(hipStreamWaitEvent(D->stream[r], X.done[(size_t)r], 0));
    return FS_OK;
  });
}

// THE ENGINE: out = M in on every rank, for any k.  whole_shard: every rank's whole local product, then run_gather -- no send
// window ever reaches into rows that are still being written.  Otherwise the local products run in parts; behind part p the event
// ev[r][p] lets the communication streams all-gather the rows the part finished (a window of maxc[p] rows from the part's first
// row into its region of the padded buffer) under the later parts, and ONE unpack per rank ends the product.  Every step is "for
// every rank do f(r)" (each_rank), so the calling thread and the issuing threads make the same calls per stream, in the same
// order.  Asynchronous: the caller waits for the compute streams (dist_sync), which wait for the unpacks (done[r]).
int run_product(fs_dist_t D, const Exchange &X, const std::vector<double *> &out, bool whole_shard, bool threads)
{
  const fs::ExchangePlan &P = X.P;
  const int n = D->n, np = P.np;
  if (whole_shard) return run_gather(D, X, X.local, out, threads, &X.whole);
  for (int p = 0; p < np; ++p) {
    std::vector<const double *> send((size_t)n);
    std::vector<double *> recv((size_t)n);
    std::vector<hipEvent_t> ready((size_t)n);
    if (int rc = each_rank(D, threads, [&](int r) -> int {
          if (int rc2 = X.part(r, p)) return rc2;
          FS_HIP(hipEventRecord(X.ev[(size_t)r][(size_t)p], D->stream[r]));
          FS_HIP(hipStreamWaitEvent(D->comm_stream[r], X.ev[(size_t)r][(size_t)p], 0));
          send[(size_t)r] = X.local[(size_t)r] + (int64_t)P.cut[(size_t)r][(size_t)p] * X.k;
          recv[(size_t)r] = X.pad[(size_t)r] + P.off[(size_t)p] * X.k;
          ready[(size_t)r] = X.ev[(size_t)r][(size_t)p];
          return FS_OK;
        })) return rc;
    // A failed exchange.  With issuing threads the error is returned: no injection, no fallback on that path.
    const bool inject = !threads && take_injection(p);
    if (int rc = exchange_equal(D, send, recv, (size_t)P.maxc[(size_t)p] * (size_t)X.k, D->comm_stream, ready, threads, inject)) {
      if (threads) return rc;
      static const bool trace = getenv("FS_TRACE_BUILD") != nullptr;
      D->conservative = true;
      if (D->use_rccl) {            // exchange_equal aborted the communicators: nothing to finish this product with
        if (trace) fprintf(stderr, "[fastsparse] the exchange of part %d failed (%s)\n", p, fs_last_error());
        return rc;
      }
      // virtual ranks (device-to-device copies, one GPU): whatever was enqueued completes by itself, so the product can be finished
      // with ONE whole-shard exchange behind the finished local product -- and the context stays conservative from now on
      if (trace) fprintf(stderr, "[fastsparse] the exchange of part %d failed (%s): conservative mode from here on\n", p, fs_last_error());
      for (int q = p + 1; q < np; ++q)
        if (int rc2 = each_rank(D, false, [&](int r) { return X.part(r, q); })) return rc2;
      if (int rc2 = dist_sync(D)) return rc2;        // whatever of the failed exchange was enqueued has drained
      return run_gather(D, X, X.local, out, false);
    }
  }
  return each_rank(D, threads, [&](int r) -> int {
    if (int rc = fs_copy_segments(P.nseg, X.table[(size_t)r] + X.table_at, P.max_seg, X.pad[(size_t)r], out[(size_t)r], D->comm_stream[r])) return rc;
    FS_HIP(hipEventRecord(X.done[(size_t)r], D->comm_stream[r]));
    FS_HIP(hipStreamWaitEvent(D->stream[r], X.done[(size_t)r], 0));   // whatever follows on the compute stream sees the whole vector
    return FS_OK;
  });
}

int dist_sync(fs_dist_t D)
{
  if (D->workers)
    return D->workers->run([D](int r) -> int {
      FS_HIP(hipStreamSynchronize(D->stream[r]));
      FS_HIP(hipStreamSynchronize(D->comm_stream[r]));
      return FS_OK;
    });
  for (int r = 0; r < D->n; ++r) {
    FS_HIP(hipSetDevice(D->dev[r]));
    FS_HIP(hipStreamSynchronize(D->stream[r]));
    FS_HIP(hipStreamSynchronize(D->comm_stream[r]));
  }
  return FS_OK;
}

// host vector -> every rank's device vector through ONE pinned staging buffer: the host copy of chunk c + 1 runs while the
// N asynchronous uploads of chunk c are in flight (each over its own PCIe link)
int upload_all(fs_dist_matrix_t M, const std::vector<double *> &dst, const double *src_host, size_t count)
{
  fs_dist_t D = M->D;
  constexpr size_t kChunk = (size_t)4 << 20;     // doubles per chunk: 32 MB
  const size_t need = std::min(count, 2 * kChunk);
  if (M->pin_doubles < need) {
    if (M->pin) (void)hipHostFree(M->pin);
    M->pin = nullptr; M->pin_doubles = 0;
    FS_HIP(hipHostMalloc(&M->pin, sizeof(double) * (need ? need : 1), hipHostMallocDefault));
    M->pin_doubles = need;
  }
  int slot = 0;
  for (size_t a = 0; a < count; a += kChunk, slot ^= 1) {
    const size_t c = std::min(kChunk, count - a);
    double *stage = M->pin + (size_t)slot * kChunk;
    if (a >= 2 * kChunk)                          // the uploads that read this half two chunks ago have to be done
      for (int r = 0; r < D->n; ++r) { FS_HIP(hipSetDevice(D->dev[r])); FS_HIP(hipStreamSynchronize(D->stream[r])); }
    memcpy(stage, src_host + a, sizeof(double) * c);
    for (int r = 0; r < D->n; ++r) {
      FS_HIP(hipSetDevice(D->dev[r]));
      FS_HIP(hipMemcpyAsync(dst[(size_t)r] + a, stage, sizeof(double) * c, hipMemcpyHostToDevice, D->stream[r]));
    }
  }
  return FS_OK;
}

int download_from(fs_dist_matrix_t M, int rank, double *dst_host, const double *src_dev, size_t count)
{
  fs_dist_t D = M->D;
  FS_HIP(hipSetDevice(D->dev[rank]));
  FS_HIP(hipMemcpyAsync(dst_host, src_dev, sizeof(double) * count, hipMemcpyDeviceToHost, D->stream[rank]));
  return FS_OK;
}

// ---- the caller's dense vectors: host memory or HBM of any device --------------------------------------------------------
// where a caller's vector lives: the HIP device ordinal, or -1 for host memory
int vector_device(const void *p)
{
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return -1; }   // plain malloc memory: not known to HIP
  return (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged) ? a.device : -1;
}

// the caller's work on the legacy default stream of device d has to be done before the ranks' (non-blocking) streams touch its
// vectors: the entry points are synchronous, like the single-GPU drop-in's
int wait_for_caller(int d)
{
  FS_HIP(hipSetDevice(d));
  FS_HIP(hipStreamSynchronize(nullptr));
  return FS_OK;
}

// The input of a product on every rank: in[r].  Host memory goes up to own[r] through the pinned staging buffer (upload_all).  A
// vector in HBM never touches the host: the ranks of ITS device read it in place (in_place), the others get it device to device
// (xGMI) into own[r].
int vec_in(fs_dist_matrix_t M, const std::vector<double *> &own, const double *src, size_t count, std::vector<double *> &in, bool in_place)
{
  fs_dist_t D = M->D;
  in = own;
  const int d = vector_device(src);
  if (d < 0) return upload_all(M, own, src, count);
  if (int rc = wait_for_caller(d)) return rc;
  for (int r = 0; r < D->n; ++r) {
    if (in_place && D->dev[r] == d) { in[(size_t)r] = const_cast<double *>(src); continue; }
    FS_HIP(hipSetDevice(D->dev[r]));
    if (count) FS_HIP(hipMemcpyPeerAsync(own[(size_t)r], D->dev[r], src, d, sizeof(double) * count, D->stream[r]));
  }
  return FS_OK;
}

// The output of a product: every rank ends up with the whole vector (out[r]).  A caller's vector in HBM IS the output vector of the
// first rank on its device (*direct), so the unpack launch writes it and nothing is copied; otherwise out = own and vec_store
// brings rank 0's copy to the caller.
int vec_out(fs_dist_matrix_t M, const std::vector<double *> &own, double *dst, std::vector<double *> &out, int *direct)
{
  fs_dist_t D = M->D;
  out = own;
  *direct = -1;
  const int d = vector_device(dst);
  if (d < 0) return FS_OK;
  if (int rc = wait_for_caller(d)) return rc;
  for (int r = 0; r < D->n && *direct < 0; ++r)
    if (D->dev[r] == d) { out[(size_t)r] = dst; *direct = r; }
  return FS_OK;
}

// count doubles from rank `rank`'s device to the caller: device to host, or device to device when dst is in HBM.  Asynchronous on
// the rank's stream (the caller's dist_sync finishes it).
int vec_store(fs_dist_matrix_t M, int rank, double *dst, const double *src_dev, size_t count)
{
  fs_dist_t D = M->D;
  if (!count) return FS_OK;
  const int d = vector_device(dst);
  if (d < 0) return download_from(M, rank, dst, src_dev, count);
  FS_HIP(hipSetDevice(D->dev[rank]));
  FS_HIP(hipMemcpyPeerAsync(dst, d, src_dev, D->dev[rank], sizeof(double) * count, D->stream[rank]));
  return FS_OK;
}

// shards of one direction from host CSR arrays (row_ptr of the direction's matrix; rp may be 64-bit for A')
template <typename RP>
int make_shards(fs_dist_t D, DistSide &S, int nrow, int ncol, const RP *row_ptr, const int *cols, const double *vals)
{
  const int n = D->n;
  S.nrow = nrow; S.ncol = ncol;
  nnz_cut(S.bounds, n, nrow, row_ptr);
  S.shard.assign((size_t)n, nullptr);
  S.shard_nnz.assign((size_t)n, 0);
  std::vector<int> lrp;
  for (int r = 0; r < n; ++r) {
    const int lo = S.bounds[(size_t)r], hi = S.bounds[(size_t)r + 1];
    const int64_t a = (int64_t)row_ptr[lo], b = (int64_t)row_ptr[hi];
    if (b - a > 0x7fffffffll) { fs::set_error("a shard holds more than 2^31-1 non-zeros: use more devices"); return FS_ERR_ARG; }
    lrp.resize((size_t)(hi - lo) + 1);
    for (int i = lo; i <= hi; ++i) lrp[(size_t)(i - lo)] = (int)((int64_t)row_ptr[i] - a);
    S.shard_nnz[(size_t)r] = b - a;
    FS_HIP(hipSetDevice(D->dev[r]));
    fs::KeepCsrScope keep_plain_arrays;     // (option release_csr is not for shards: the exchange layer's own later work -- A' on the
                                            //  devices, a k-column prepare -- reads them)
    S.shard[(size_t)r] = fs_csr_create(hi - lo, ncol, b - a, lrp.data(), cols ? cols + a : nullptr, vals ? vals + a : nullptr, FS_HOST, 0);
    if (!S.shard[(size_t)r]) return FS_ERR_HIP;
  }
  return plan_side(D, S, env_parts());
}

// a side whose last owner -- the matrix it was made for, or a pair that shares it (fs_dist_matrix_pair) -- frees its shards
std::shared_ptr<DistSide> side_owner(fs_dist_t D)
{
  return std::shared_ptr<DistSide>(new DistSide(), [D](DistSide *S) {
    DeviceGuard guard;
    (void)dist_sync(D);
    free_side(D, *S);
    delete S;
  });
}

fs_dist_matrix_t new_dist_matrix(fs_dist_t D, int nrow, int ncol, std::shared_ptr<DistSide> A = nullptr, std::shared_ptr<DistSide> T = nullptr)
{
  fs_dist_matrix_t M = new fs_dist_matrix_s(A ? A : side_owner(D), T ? T : side_owner(D));
  M->D = D; M->nrow = nrow; M->ncol = ncol;
  const int n = D->n;
  M->x.assign((size_t)n, nullptr);
  M->y.assign((size_t)n, nullptr);
  M->z.assign((size_t)n, nullptr);
  return M;
}

bool alloc_xy(fs_dist_matrix_t M)
{
  fs_dist_t D = M->D;
  bool ok = true;
  for (int r = 0; ok && r < D->n; ++r) {
    ok = hipSetDevice(D->dev[r]) == hipSuccess;
    ok = ok && hipMalloc(&M->x[(size_t)r], sizeof(double) * (size_t)(M->ncol ? M->ncol : 1)) == hipSuccess;
    ok = ok && hipMalloc(&M->y[(size_t)r], sizeof(double) * (size_t)(M->nrow ? M->nrow : 1)) == hipSuccess;
    if (!ok) fs::set_error("fs_dist: out of device memory for the replicated vectors");
  }
  return ok;
}

// after the shards of A' exist: their plan and the z vectors
int finish_transpose(fs_dist_matrix_t M)
{
  fs_dist_t D = M->D;
  DistSide &T = M->t;
  int rc = plan_side(D, T, env_parts());
  for (int r = 0; rc == FS_OK && r < D->n; ++r) {
    if (hipSetDevice(D->dev[r]) != hipSuccess || hipMalloc(&M->z[(size_t)r], sizeof(double) * (size_t)(M->ncol ? M->ncol : 1)) != hipSuccess) {
      fs::set_error("fs_dist_matrix_build_transpose: out of device memory");
      rc = FS_ERR_HIP;
    }
  }
  if (rc != FS_OK) {
    for (int r = 0; r < D->n; ++r)
      if (M->z[(size_t)r]) { (void)hipSetDevice(D->dev[r]); (void)hipFree(M->z[(size_t)r]); M->z[(size_t)r] = nullptr; }
    free_side(D, T);
  }
  return rc;
}

// buffers, tables and prepared shards for products with k row-major columns (k >= 2); idempotent per (k, transposed side built)
int ensure_k(fs_dist_matrix_t M, int k)
{
  fs_dist_t D = M->D;
  const int n = D->n;
  KWork &W = M->kw;
  const bool with_t = M->t.built;
  if (W.mem.ready && W.k == k && W.with_t == with_t && W.epoch == fs::option_epoch()) return FS_OK;
  if (int rc = dist_sync(D)) return rc;
  free_work(D, W);
  W.k = k; W.with_t = with_t; W.epoch = fs::option_epoch();
  // the k-column copies of the shards first (fs_spmm itself never builds): the parts below belong to the plan they leave
  for (int r = 0; r < n; ++r) {
    FS_HIP(hipSetDevice(D->dev[r]));
    if (M->a.shard[(size_t)r])
      if (int rc = fs_matrix_prepare(M->a.shard[(size_t)r], k, 0, D->stream[r])) return rc;
    if (with_t && M->t.shard[(size_t)r])
      if (int rc = fs_matrix_prepare(M->t.shard[(size_t)r], k, 0, D->stream[r])) return rc;
  }
  if (int rc = side_plan(D, M->a, k, M->a.plan.np > 0 ? M->a.plan.np : 1, W.pa)) return rc;
  if (with_t)
    if (int rc = side_plan(D, M->t, k, M->t.plan.np > 0 ? M->t.plan.np : 1, W.pt)) return rc;
  std::vector<int64_t> tab(W.pa.table);
  tab.insert(tab.end(), W.pt.table.begin(), W.pt.table.end());
  const size_t pad_rows = (size_t)std::max(W.pa.pad_rows, W.pt.pad_rows);
  const size_t F = (size_t)(M->ncol ? M->ncol : 1) * k, N = (size_t)(M->nrow ? M->nrow : 1) * k;
  return W.mem.fill(D, [&](int r) -> int {
    if (int rc = W.mem.get(r, W.x, F)) return rc;
    if (int rc = W.mem.get(r, W.y, N)) return rc;
    if (int rc = W.mem.get(r, W.z, F)) return rc;
    if (int rc = W.mem.get(r, W.la, (size_t)W.pa.local_rows * k)) return rc;
    if (int rc = W.mem.get(r, W.lt, (size_t)W.pt.local_rows * k)) return rc;      // (one row when A' is not built)
    if (int rc = W.mem.get(r, W.pad, (pad_rows + 1) * k)) return rc;
    if (int rc = W.mem.get(r, W.tab, tab.size() + 1)) return rc;
    if (!tab.empty()) FS_HIP(hipMemcpy(W.tab[(size_t)r], tab.data(), sizeof(int64_t) * tab.size(), hipMemcpyHostToDevice));
    if (int rc = W.mem.get(r, W.sol, F)) return rc;
    if (int rc = W.mem.get(r, W.r, F)) return rc;
    if (int rc = W.mem.get(r, W.b, F)) return rc;
    if (int rc = W.mem.get(r, W.part, (size_t)fs::kCgPartDoubles)) return rc;
    if (int rc = W.mem.get(r, W.red, 4)) return rc;
    return W.mem.get(r, W.st, (size_t)fs::kCgStateDoubles);
  });
}

// one side of the matrix as the engine sees it: k = 1 on the side's own plan and buffers, k > 1 (after ensure_k(M, k)) on KWork's
Exchange exchange_of(fs_dist_matrix_t M, bool transposed, int k)
{
  DistSide &S = transposed ? M->t : M->a;
  KWork &W = M->kw;
  if (k == 1) return Exchange{S.plan, 1, S.local, S.pad, S.table, 0, S.ev, S.done, nullptr, nullptr};
  return Exchange{transposed ? W.pt : W.pa, k, transposed ? W.lt : W.la, W.pad, W.tab, transposed ? W.pa.table.size() : 0, S.ev, S.done, nullptr, nullptr};
}

// out = M in (M: A, or A' when `transposed`) for k row-major columns on every rank, through the one engine (run_product).  in[r] /
// out[r]: the replicated input and the gathered output on rank r's device.  What differs between k = 1 and k > 1 is here:
int dist_product(fs_dist_matrix_t M, bool transposed, int k, const std::vector<double *> &in, const std::vector<double *> &out)
{
  fs_dist_t D = M->D;
  DistSide &S = transposed ? M->t : M->a;
  if (int rc = context_usable(D)) return rc;         // the broken check first, then every product counts once
  ++g_products;
  if (k == 1)                                        // the cuts of the single-vector product follow the options; the k-column plan
    if (int rc = replan_if_moved(D, S)) return rc;   // is rebuilt by ensure_k on any epoch change
  Exchange X = exchange_of(M, transposed, k);
  const int np = X.P.np;
  const std::vector<double *> &local = X.local;
  auto rows = [&S](int r) { return S.bounds[(size_t)r + 1] - S.bounds[(size_t)r]; };
  X.part = [&, k, np](int r, int p) -> int {
    if (rows(r) <= 0) return FS_OK;
    return k == 1 ? fs_spmv_part(S.shard[(size_t)r], 0, local[(size_t)r], in[(size_t)r], p, np, D->stream[r])
                  : fs_spmm_part(S.shard[(size_t)r], 0, local[(size_t)r], in[(size_t)r], k, p, np, D->stream[r]);
  };
  // whole-shard mode launches the single-vector product as all np calls of fs_spmv_part (the two-pass pair by ranges of panels
  // IS the product), the k-column product as ONE fs_spmm (whatever plan the prepare left: row kernel, column sweeps, one sweep)
  X.whole = [&, k, np](int r) -> int {
    if (rows(r) <= 0) return FS_OK;
    if (k > 1) return fs_spmm(S.shard[(size_t)r], local[(size_t)r], in[(size_t)r], k, D->stream[r]);
    for (int p = 0; p < np; ++p)
      if (int rc = fs_spmv_part(S.shard[(size_t)r], 0, local[(size_t)r], in[(size_t)r], p, np, D->stream[r])) return rc;
    return FS_OK;
  };
  // k > 1 also goes whole-shard when no rank finishes rows in more than one part (!real: every plan but the one sweep of k = 2, 4):
  // np all-gathers would hide nothing.  k = 1 asks only for the part count.
  const bool whole_shard = D->conservative || np <= 1 || (k > 1 && !X.P.real);
  // FS_DIST_THREADS=1 moves only the k = 1 products to the issuing threads; the k-column products have always been issued by the
  // calling thread.  An inherited asymmetry, not a decision.
  const bool threads = D->workers != nullptr && k == 1;
  return run_product(D, X, out, whole_shard, threads);
}

}  // namespace

extern "C" {

fs_dist_t fs_dist_create(int ndev, const int *devices)
{
  int visible = 0;
  if (hipGetDeviceCount(&visible) != hipSuccess || visible < 1) { fs::set_error("fs_dist_create: no HIP device"); return nullptr; }
  if (ndev < 1) ndev = visible;
  if (ndev > 64) { fs::set_error("fs_dist_create: at most 64 ranks"); return nullptr; }
  DeviceGuard guard;
  fs_dist_t D = new fs_dist_s();
  D->n = ndev;
  D->conservative = env_parts() == 1;
  bool distinct = true;
  for (int r = 0; r < ndev; ++r) {
    const int d = devices ? devices[r] : r;
    if (d < 0 || d >= visible) { fs::set_error("fs_dist_create: device out of range"); delete D; return nullptr; }
    for (int q : D->dev) distinct = distinct && q != d;
    D->dev.push_back(d);
  }
  for (int r = 0; r < ndev; ++r) {
    hipStream_t s = nullptr, c = nullptr;
    if (hipSetDevice(D->dev[r]) != hipSuccess || hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c, hipStreamNonBlocking) != hipSuccess) {
      fs::set_error("fs_dist_create: cannot create a stream");
      if (s) (void)hipStreamDestroy(s);
      fs_dist_destroy(D);
      return nullptr;
    }
    D->stream.push_back(s);
    D->comm_stream.push_back(c);
  }
  // FS_DIST_FORCE_RCCL=1 also takes a one-device context through RCCL (communicator, group call, collective on the
  // rank's communication stream): the only way to run that code on a one-GPU machine
  const char *force = getenv("FS_DIST_FORCE_RCCL");
  if (distinct && (ndev > 1 || (force && *force == '1'))) {
    if (!rccl().ok) { fs::set_error("fs_dist_create: librccl.so could not be loaded"); fs_dist_destroy(D); return nullptr; }
    D->comm.assign((size_t)ndev, nullptr);
    const ncclResult_t e = rccl().CommInitAll(D->comm.data(), ndev, D->dev.data());
    if (e != ncclSuccess) { nccl_fail(e, "ncclCommInitAll"); D->comm.clear(); fs_dist_destroy(D); return nullptr; }
    D->use_rccl = true;
  }
  if (const char *t = getenv("FS_DIST_THREADS"))
    if (*t == '1' && ndev > 1) {
      D->workers.reset(new RankWorkers());
      D->workers->start(D->dev);
    }
  return D;
}

void fs_dist_destroy(fs_dist_t D)
{
  if (!D) return;
  DeviceGuard guard;
  for (ncclComm_t c : D->comm)
    if (c) (void)rccl().CommDestroy(c);
  for (size_t r = 0; r < D->stream.size(); ++r) {
    (void)hipSetDevice(D->dev[r]);
    (void)hipStreamDestroy(D->stream[r]);
    if (r < D->comm_stream.size()) (void)hipStreamDestroy(D->comm_stream[r]);
  }
  delete D;
}

long fs_debug_dist_products(void) { return g_products.load(); }   // diagnostics, not in include/fastsparse_hip.h

// in how many parts the k-column product of the handle's current k finishes rows (the most any rank has; 1: the exchange simply
// follows the product; 0: no k-column product was made yet)
int fs_debug_dist_k_parts(fs_dist_matrix_t M, int transposed)
{
  if (!M || !M->kw.mem.ready) return 0;
  return fs::most_busy_parts((transposed ? M->kw.pt : M->kw.pa).cut);
}

// the same for the single-vector product of one side (0: no product made on that side yet)
int fs_debug_dist_parts(fs_dist_matrix_t M, int transposed)
{
  if (!M) return 0;
  const DistSide &S = transposed ? M->t : M->a;
  return S.built ? fs::most_busy_parts(S.plan.cut) : 0;
}

int fs_dist_ndev(fs_dist_t D) { return D ? D->n : FS_ERR_ARG; }
int fs_dist_uses_rccl(fs_dist_t D) { return D ? (int)D->use_rccl : FS_ERR_ARG; }
int fs_debug_dist_issue_threads(fs_dist_t D) { return D && D->workers ? D->workers->n : 0; }   // diagnostics
int fs_dist_is_conservative(fs_dist_t D) { return D ? (int)D->conservative : FS_ERR_ARG; }

void fs_dist_matrix_destroy(fs_dist_matrix_t M)
{
  if (!M) return;
  DeviceGuard guard;
  (void)dist_sync(M->D);
  free_work(M->D, M->cg);
  free_work(M->D, M->pn);
  free_work(M->D, M->ms);
  free_work(M->D, M->mn);
  free_work(M->D, M->kw);
  for (size_t r = 0; r < (size_t)M->D->n; ++r) {
    (void)hipSetDevice(M->D->dev[r]);
    if (r < M->x.size() && M->x[r]) (void)hipFree(M->x[r]);
    if (r < M->y.size() && M->y[r]) (void)hipFree(M->y[r]);
    if (r < M->z.size() && M->z[r]) (void)hipFree(M->z[r]);
  }
  if (M->pin) (void)hipHostFree(M->pin);
  delete M;          // the sides go with their last owner (side_owner)
}

fs_dist_matrix_t fs_dist_csr_create(fs_dist_t D, int nrow, int ncol, int64_t nnz, const int *row_ptr, const int *cols,
                                    const double *vals)
{
  if (!D || nrow < 0 || ncol < 0 || nnz < 0 || !row_ptr || (nnz > 0 && !cols)) { fs::set_error("fs_dist_csr_create: bad argument"); return nullptr; }
  DeviceGuard guard;
  fs_dist_matrix_t M = new_dist_matrix(D, nrow, ncol);
  M->nnz = nnz;
  const bool ok = make_shards(D, M->a, nrow, ncol, row_ptr, cols, vals) == FS_OK && alloc_xy(M);
  if (!ok) { fs_dist_matrix_destroy(M); return nullptr; }
  return M;
}

// host COO arrays (optionally valued) -> the same row shards: the entries are bucketed stably by row first -- new_csr / new_bcsr
// (csr.h:375-422, 30-67; on the device from 4 M entries, fs_bucket_coo) -- so every row keeps the caller's entry order, the order
// the serial COO loops add in (sparse.h:58-65, dsparse.h:43-51): what fs_coo_create does on one GPU.  A_mul_B / sdm_A_mul_B /
// bsbm_* / bsdm_* across the GPUs enter here; At_mul_B passes (cols, rows).
fs_dist_matrix_t fs_dist_coo_create(fs_dist_t D, int nrow, int ncol, int64_t nnz, const int *rows, const int *cols, const double *vals)
{
  if (!D || nrow < 0 || ncol < 0 || nnz < 0 || nnz > 0x7fffffffll || (nnz > 0 && (!rows || !cols))) {
    fs::set_error("fs_dist_coo_create: bad argument (0 .. 2^31-1 entries)");
    return nullptr;
  }
  for (int64_t i = 0; i < nnz; ++i)
    if ((unsigned)rows[i] >= (unsigned)nrow) { fs::set_error("fs_dist_coo_create: row out of range"); return nullptr; }
  fs_dist_matrix_t M = nullptr;
  if (vals) {
    struct CSR c;
    new_csr(&c, (long)nnz, nrow, ncol, const_cast<int *>(rows), const_cast<int *>(cols), const_cast<double *>(vals));
    M = fs_dist_csr_create(D, nrow, ncol, nnz, c.row_ptr, c.cols, c.vals);
    free(c.row_ptr); free(c.cols); free(c.vals);
  } else {
    struct BinaryCSR c;
    new_bcsr(&c, (long)nnz, nrow, ncol, const_cast<int *>(rows), const_cast<int *>(cols));
    M = fs_dist_csr_create(D, nrow, ncol, nnz, c.row_ptr, c.cols, nullptr);
    free(c.row_ptr); free(c.cols);
  }
  return M;
}

// A and A' as the caller holds them -- two matrices (bsbm_cg(x, B, Bt, ...), cg.h:25: B and the blocked form of its transpose) --
// as ONE handle for fs_dist_cg / fs_dist_cg2 / fs_dist_ata / the *_t products: its direct side is A's, its transposed side is At's
// DIRECT side (so a row of A' adds in the order the caller's own At stores it, like the single-GPU solvers on two handles).
// Nothing is copied: the shards are shared with A and At and live until the last of the three handles is destroyed.  The pair
// has its own vectors and solver work space.
fs_dist_matrix_t fs_dist_matrix_pair(fs_dist_matrix_t A, fs_dist_matrix_t At)
{
  if (!A || !At || A->D != At->D) { fs::set_error("fs_dist_matrix_pair: NULL handle, or handles of two contexts"); return nullptr; }
  if (A->nrow != At->ncol || A->ncol != At->nrow) { fs::set_error("fs_dist_matrix_pair: the matrices are not each other's transposes in shape"); return nullptr; }
  DeviceGuard guard;
  std::lock_guard<std::mutex> ga(A->lock);
  fs_dist_matrix_t M = new_dist_matrix(A->D, A->nrow, A->ncol, A->pa, At->pa);
  M->nnz = A->nnz;
  bool ok = alloc_xy(M);
  for (int r = 0; ok && r < A->D->n; ++r)
    ok = hipSetDevice(A->D->dev[r]) == hipSuccess && hipMalloc(&M->z[(size_t)r], sizeof(double) * (size_t)(M->ncol ? M->ncol : 1)) == hipSuccess;
  if (!ok) { fs::set_error("fs_dist_matrix_pair: out of device memory for the vectors"); fs_dist_matrix_destroy(M); return nullptr; }
  return M;
}

// The matrix as the caller already holds it: one CSR per rank -- shard r = rows [sum of shard_rows[0 .. r), + shard_rows[r]) of
// A with a LOCAL row_ptr (shard_rows[r] + 1 ints, starting at 0), GLOBAL column ids and optional values.  Nothing here ever
// sees the whole matrix, so the total number of entries may exceed 2^31 - 1 (every shard stays below: int row_ptr,
// csr.h:358-366) -- BASELINE config 5 (3.2 G entries) comes in this way.  space = FS_HOST: host arrays; FS_DEVICE: shard r's
// arrays live on rank r's device (they are copied: the caller may free them).  The caller chooses the cuts (balance by
// non-zeros for power-law matrices).
fs_dist_matrix_t fs_dist_csr_create_from_shards(fs_dist_t D, int nrow, int ncol, const int *shard_rows, const int64_t *shard_nnz,
                                                const int *const *row_ptr, const int *const *cols, const double *const *vals, int space)
{
  if (!D || nrow < 0 || ncol < 0 || !shard_rows || !shard_nnz || !row_ptr || !cols) { fs::set_error("fs_dist_csr_create_from_shards: bad argument"); return nullptr; }
  const int n = D->n;
  int64_t rows = 0, nnz = 0;
  for (int r = 0; r < n; ++r) {
    if (shard_rows[r] < 0 || shard_nnz[r] < 0 || shard_nnz[r] > 0x7fffffffll || !row_ptr[r] || (shard_nnz[r] > 0 && !cols[r])) {
      fs::set_error("fs_dist_csr_create_from_shards: bad shard (each holds 0 .. 2^31-1 entries)");
      return nullptr;
    }
    rows += shard_rows[r];
    nnz += shard_nnz[r];
  }
  if (rows != nrow) { fs::set_error("fs_dist_csr_create_from_shards: the shards' rows do not add up to nrow"); return nullptr; }
  // valued or pattern-only: what the first NON-EMPTY shard says (the caller chooses the cuts: an empty first shard is legal, and an
  // empty shard's vals pointer means nothing)
  bool valued = false;
  for (int r = 0; r < n; ++r)
    if (shard_nnz[r] > 0) { valued = vals && vals[r] != nullptr; break; }
  for (int r = 0; r < n; ++r)
    if (shard_nnz[r] > 0 && (valued != (vals && vals[r] != nullptr))) { fs::set_error("fs_dist_csr_create_from_shards: values for some shards only"); return nullptr; }
  DeviceGuard guard;
  // a shard's row_ptr must end at its shard_nnz (the device kernels trust both): one int per shard, read where it lives
  for (int r = 0; r < n; ++r) {
    int last = 0;
    if (space == FS_DEVICE) {
      if (hipSetDevice(D->dev[r]) != hipSuccess || hipMemcpy(&last, row_ptr[r] + shard_rows[r], sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        fs::set_error("fs_dist_csr_create_from_shards: cannot read a shard's row_ptr on its device");
        return nullptr;
      }
    } else last = row_ptr[r][shard_rows[r]];
    if ((int64_t)last != shard_nnz[r]) { fs::set_error("fs_dist_csr_create_from_shards: row_ptr[shard_rows] of a shard is not its shard_nnz"); return nullptr; }
  }
  fs_dist_matrix_t M = new_dist_matrix(D, nrow, ncol);
  M->nnz = nnz;
  DistSide &S = M->a;
  S.nrow = nrow; S.ncol = ncol;
  S.bounds.assign((size_t)n + 1, 0);
  S.shard.assign((size_t)n, nullptr);
  S.shard_nnz.assign((size_t)n, 0);
  bool ok = true;
  for (int r = 0; ok && r < n; ++r) {
    S.bounds[(size_t)r + 1] = S.bounds[(size_t)r] + shard_rows[r];
    S.shard_nnz[(size_t)r] = shard_nnz[r];
    ok = hipSetDevice(D->dev[r]) == hipSuccess;
    fs::KeepCsrScope keep_plain_arrays;     // (option release_csr is not for shards: the exchange layer's own later work -- A' on the
                                            //  devices, a k-column prepare -- reads them)
    if (ok) S.shard[(size_t)r] = fs_csr_create(shard_rows[r], ncol, shard_nnz[r], row_ptr[r], cols[r], valued ? vals[r] : nullptr, space, 0);
    ok = ok && S.shard[(size_t)r] != nullptr;
  }
  ok = ok && plan_side(D, S, env_parts()) == FS_OK && alloc_xy(M);
  if (!ok) { fs_dist_matrix_destroy(M); return nullptr; }
  return M;
}

// Row shards of A' (cut by non-zeros of the COLUMNS of A) from the same host arrays the matrix was created from: one pass
// counts the columns, one pass per device -- in parallel, one host thread each -- collects its columns' entries in ascending
// row order (the order a stable column sort of A gives: rows of A' keep it, like fs_matrix_build_transpose on one GPU).
int fs_dist_matrix_build_transpose(fs_dist_matrix_t M, const int *row_ptr, const int *cols, const double *vals)
{
  if (!M || !row_ptr || (M->nnz > 0 && !cols)) { fs::set_error("fs_dist_matrix_build_transpose: bad argument"); return FS_ERR_ARG; }
  std::lock_guard<std::mutex> g(M->lock);
  if (M->t.built) return FS_OK;
  DeviceGuard guard;
  fs_dist_t D = M->D;
  const int n = D->n, nrow = M->nrow, ncol = M->ncol;
  std::vector<int64_t> tptr((size_t)ncol + 1, 0);           // row_ptr of A'
  for (int64_t i = 0; i < M->nnz; ++i) {
    if ((unsigned)cols[i] >= (unsigned)ncol) { fs::set_error("fs_dist_matrix_build_transpose: column out of range"); return FS_ERR_ARG; }
    ++tptr[(size_t)cols[i] + 1];
  }
  for (int c = 0; c < ncol; ++c) tptr[(size_t)c + 1] += tptr[(size_t)c];
  DistSide &T = M->t;
  T.nrow = ncol; T.ncol = nrow;
  nnz_cut(T.bounds, n, ncol, tptr.data());
  T.shard.assign((size_t)n, nullptr);
  T.shard_nnz.assign((size_t)n, 0);
  std::vector<int> rcs((size_t)n, FS_OK);
  std::vector<std::string> errs((size_t)n);
  std::mutex create_lock;                                    // the host passes run in parallel, the device builds one at a time
  std::vector<std::thread> th;
  for (int r = 0; r < n; ++r)
    th.emplace_back([&, r] {
      const int lo = T.bounds[(size_t)r], hi = T.bounds[(size_t)r + 1];
      const int64_t base = tptr[(size_t)lo], cnt = tptr[(size_t)hi] - base;
      T.shard_nnz[(size_t)r] = cnt;
      if (cnt > 0x7fffffffll) { rcs[(size_t)r] = FS_ERR_ARG; errs[(size_t)r] = "a shard of A' holds more than 2^31-1 non-zeros"; return; }
      std::vector<int> lrp((size_t)(hi - lo) + 1), lc((size_t)cnt);
      std::vector<double> lv(vals ? (size_t)cnt : 0);
      for (int c = lo; c <= hi; ++c) lrp[(size_t)(c - lo)] = (int)(tptr[(size_t)c] - base);
      std::vector<int> fill(lrp.begin(), lrp.end() - 1);
      for (int row = 0; row < nrow; ++row)
        for (int64_t i = row_ptr[row]; i < row_ptr[row + 1]; ++i) {
          const int c = cols[i];
          if (c < lo || c >= hi) continue;
          const int at = fill[(size_t)(c - lo)]++;
          lc[(size_t)at] = row;
          if (vals) lv[(size_t)at] = vals[i];
        }
      std::lock_guard<std::mutex> cg(create_lock);
      if (hipSetDevice(D->dev[r]) != hipSuccess) { rcs[(size_t)r] = FS_ERR_HIP; errs[(size_t)r] = "hipSetDevice failed"; return; }
      fs::KeepCsrScope keep_plain_arrays;     // (option release_csr is not for shards: the exchange layer's own later work -- A' on the
                                              //  devices, a k-column prepare -- reads them)
      T.shard[(size_t)r] = fs_csr_create(hi - lo, nrow, cnt, lrp.data(), lc.data(), vals ? lv.data() : nullptr, FS_HOST, 0);
      if (!T.shard[(size_t)r]) { rcs[(size_t)r] = FS_ERR_HIP; errs[(size_t)r] = fs_last_error(); }
    });
  for (std::thread &t : th) t.join();
  int rc = FS_OK;
  for (int r = 0; r < n; ++r)
    if (rcs[(size_t)r] != FS_OK) { rc = rcs[(size_t)r]; fs::set_error("fs_dist_matrix_build_transpose: " + errs[(size_t)r]); }
  if (rc != FS_OK) { free_side(D, T); return rc; }
  return finish_transpose(M);
}

// The same shards of A' with no host array of the matrix anywhere: built from the device-resident shards of A.
//   1  every rank counts its entries per column; the counts are added up on rank 0's device and cut by non-zeros there
//      (the cut of nnz_cut: the same bounds fs_dist_matrix_build_transpose finds on the host);
//   2  every rank partitions its entries stably by the rank that will own their column (fs::shard_transpose_partition);
//   3  the parts travel device to device (hipMemcpyPeerAsync: one process, so no collective is needed for a one-time build;
//      with virtual ranks these are copies inside one device), concatenated per destination in source-rank order;
//   4  every rank orders what it received by row of A' -- fs_coo_create's stable sort -- which leaves each row of A' in
//      ascending A-row order.
// Temporary HBM per rank: about 30 bytes per entry sent plus 16 per entry received.  Idempotent.
int fs_dist_matrix_build_transpose_device(fs_dist_matrix_t M)
{
  if (!M) { fs::set_error("fs_dist_matrix_build_transpose_device: NULL handle"); return FS_ERR_ARG; }
  std::lock_guard<std::mutex> g(M->lock);
  if (M->t.built) return FS_OK;
  DeviceGuard guard;
  fs_dist_t D = M->D;
  const int n = D->n, nrow = M->nrow, ncol = M->ncol;
  if (int rc = dist_sync(D)) return rc;
  const bool valued = [&] { for (int r = 0; r < n; ++r) if (M->a.shard_nnz[(size_t)r] > 0) return M->a.shard[(size_t)r]->a.has_vals(); return false; }();
  for (int r = 0; r < n; ++r)
    if (M->a.shard[(size_t)r])
      if (int rc = fs::need_plain_csr(M->a.shard[(size_t)r]->a, "fs_dist_matrix_build_transpose_device")) return rc;
  DistSide &T = M->t;
  T.nrow = ncol; T.ncol = nrow;
  T.bounds.assign((size_t)n + 1, 0);
  T.shard.assign((size_t)n, nullptr);
  T.shard_nnz.assign((size_t)n, 0);
  struct Tmp {
    fs_dist_t D;
    std::vector<int *> cnt, trow, tcol, rrow, rcol;
    std::vector<double *> tval, rval;
    ~Tmp()
    {
      for (size_t r = 0; r < cnt.size(); ++r) {
        (void)hipSetDevice(D->dev[r]);
        for (void *p : {(void *)cnt[r], (void *)trow[r], (void *)tcol[r], (void *)rrow[r], (void *)rcol[r], (void *)tval[r], (void *)rval[r]})
          if (p) (void)hipFree(p);
      }
    }
  } W{D};
  W.cnt.assign((size_t)n, nullptr); W.trow.assign((size_t)n, nullptr); W.tcol.assign((size_t)n, nullptr);
  W.rrow.assign((size_t)n, nullptr); W.rcol.assign((size_t)n, nullptr);
  W.tval.assign((size_t)n, nullptr); W.rval.assign((size_t)n, nullptr);
  // 1: column counts, added up on rank 0's device
  const size_t cbytes = sizeof(int) * (size_t)(ncol ? ncol : 1);
  for (int r = 0; r < n; ++r) {
    FS_HIP(hipSetDevice(D->dev[r]));
    FS_HIP(hipMalloc(&W.cnt[(size_t)r], cbytes));
    FS_HIP(hipMemsetAsync(W.cnt[(size_t)r], 0, cbytes, D->stream[r]));
    if (int rc = fs::shard_column_counts(M->a.shard[(size_t)r]->a, W.cnt[(size_t)r], D->stream[r])) return rc;
  }
  if (int rc = dist_sync(D)) return rc;
  {
    int *tmp = nullptr;
    FS_HIP(hipSetDevice(D->dev[0]));
    if (n > 1) FS_HIP(hipMalloc(&tmp, cbytes));
    int rc = FS_OK;
    for (int r = 1; r < n && rc == FS_OK; ++r) {
      if (hipMemcpyPeerAsync(tmp, D->dev[0], W.cnt[(size_t)r], D->dev[r], cbytes, D->stream[0]) != hipSuccess) { fs::set_error("fs_dist_matrix_build_transpose_device: peer copy of the column counts failed"); rc = FS_ERR_HIP; break; }
      rc = fs::add_counts(ncol, W.cnt[0], tmp, D->stream[0]);
    }
    int64_t total = 0;
    if (rc == FS_OK) rc = fs::cut_by_counts(ncol, W.cnt[0], n, T.bounds.data(), &total, D->stream[0]);
    if (tmp) (void)hipFree(tmp);
    if (rc != FS_OK) { T = DistSide(); return rc; }
    if (total != M->nnz) { fs::set_error("fs_dist_matrix_build_transpose_device: the column counts do not add up to nnz"); T = DistSide(); return FS_ERR_ARG; }
  }
  // 2: every rank's entries by destination
  std::vector<std::vector<int64_t>> count((size_t)n, std::vector<int64_t>((size_t)n, 0));   // [source][destination]
  for (int r = 0; r < n; ++r) {
    FS_HIP(hipSetDevice(D->dev[r]));
    (void)hipFree(W.cnt[(size_t)r]); W.cnt[(size_t)r] = nullptr;
    if (int rc = fs::shard_transpose_partition(M->a.shard[(size_t)r]->a, M->a.bounds[(size_t)r], n, T.bounds.data(), &W.trow[(size_t)r], &W.tcol[(size_t)r],
                                               &W.tval[(size_t)r], count[(size_t)r].data(), D->stream[r])) { T = DistSide(); return rc; }
  }
  // 3: the exchange
  for (int d = 0; d < n; ++d) {
    int64_t cnt = 0;
    for (int r = 0; r < n; ++r) cnt += count[(size_t)r][(size_t)d];
    T.shard_nnz[(size_t)d] = cnt;
    if (cnt > 0x7fffffffll) { fs::set_error("fs_dist_matrix_build_transpose_device: a shard of A' holds more than 2^31-1 non-zeros: use more devices"); T = DistSide(); return FS_ERR_ARG; }
    FS_HIP(hipSetDevice(D->dev[d]));
    const size_t c1 = (size_t)(cnt ? cnt : 1);
    FS_HIP(hipMalloc(&W.rrow[(size_t)d], sizeof(int) * c1));
    FS_HIP(hipMalloc(&W.rcol[(size_t)d], sizeof(int) * c1));
    if (valued) FS_HIP(hipMalloc(&W.rval[(size_t)d], sizeof(double) * c1));
  }
  for (int r = 0; r < n; ++r) {
    FS_HIP(hipSetDevice(D->dev[r]));
    int64_t soff = 0;
    for (int d = 0; d < n; ++d) {
      const int64_t c = count[(size_t)r][(size_t)d];
      int64_t doff = 0;
      for (int q = 0; q < r; ++q) doff += count[(size_t)q][(size_t)d];
      if (c > 0) {
        FS_HIP(hipMemcpyPeerAsync(W.rrow[(size_t)d] + doff, D->dev[d], W.trow[(size_t)r] + soff, D->dev[r], sizeof(int) * (size_t)c, D->stream[r]));
        FS_HIP(hipMemcpyPeerAsync(W.rcol[(size_t)d] + doff, D->dev[d], W.tcol[(size_t)r] + soff, D->dev[r], sizeof(int) * (size_t)c, D->stream[r]));
        if (valued) FS_HIP(hipMemcpyPeerAsync(W.rval[(size_t)d] + doff, D->dev[d], W.tval[(size_t)r] + soff, D->dev[r], sizeof(double) * (size_t)c, D->stream[r]));
      }
      soff += c;
    }
  }
  if (int rc = dist_sync(D)) { T = DistSide(); return rc; }
  // 4: the local builds
  for (int d = 0; d < n; ++d) {
    FS_HIP(hipSetDevice(D->dev[d]));
    for (void **p : {(void **)&W.trow[(size_t)d], (void **)&W.tcol[(size_t)d], (void **)&W.tval[(size_t)d]})
      if (*p) { (void)hipFree(*p); *p = nullptr; }
    fs::KeepCsrScope keep_plain_arrays;     // (option release_csr is not for shards: the exchange layer's own later work -- A' on the
                                            //  devices, a k-column prepare -- reads them)
    T.shard[(size_t)d] = fs_coo_create(T.bounds[(size_t)d + 1] - T.bounds[(size_t)d], nrow, T.shard_nnz[(size_t)d], W.rrow[(size_t)d], W.rcol[(size_t)d],
                                       valued ? W.rval[(size_t)d] : nullptr, FS_DEVICE);
    if (!T.shard[(size_t)d]) { free_side(D, T); return FS_ERR_HIP; }
    for (void **p : {(void **)&W.rrow[(size_t)d], (void **)&W.rcol[(size_t)d], (void **)&W.rval[(size_t)d]})
      if (*p) { (void)hipFree(*p); *p = nullptr; }
  }
  return finish_transpose(M);
}

int fs_dist_matrix_has_transpose(fs_dist_matrix_t M) { return M && M->t.built; }

int fs_dist_matrix_bounds(fs_dist_matrix_t M, int *bounds)
{
  if (!M || !bounds) return FS_ERR_ARG;
  for (size_t i = 0; i < M->a.bounds.size(); ++i) bounds[i] = M->a.bounds[i];
  return FS_OK;
}

int fs_dist_matrix_bounds_t(fs_dist_matrix_t M, int *bounds)
{
  if (!M || !bounds || !M->t.built) return FS_ERR_ARG;
  for (size_t i = 0; i < M->t.bounds.size(); ++i) bounds[i] = M->t.bounds[i];
  return FS_OK;
}

int64_t fs_dist_matrix_shard_nnz(fs_dist_matrix_t M, int rank)
{
  if (!M || rank < 0 || rank >= M->D->n) return FS_ERR_ARG;
  return M->a.shard_nnz[(size_t)rank];
}

int64_t fs_dist_matrix_nnz(fs_dist_matrix_t M) { return M ? M->nnz : FS_ERR_ARG; }

fs_matrix_t fs_dist_matrix_shard(fs_dist_matrix_t M, int rank, int transposed)
{
  if (!M || rank < 0 || rank >= M->D->n || (transposed && !M->t.built)) return nullptr;
  return (transposed ? M->t : M->a).shard[(size_t)rank];
}

// Y[rows of M, k] = M X, row-major, with the caller's vectors in host memory or in HBM (vec_in / vec_out): one direction of the
// matrix.  k = 1 works on the handle's x / y / z, k > 1 on the k-column work space (prepared on first use of a k: ensure_k).
static int dist_apply(fs_dist_matrix_t M, bool transposed, double *y, const double *x, int k)
{
  std::lock_guard<std::mutex> g(M->lock);
  std::lock_guard<std::mutex> gd(M->D->lock);
  DeviceGuard guard;
  if (k > 1)
    if (int rc = ensure_k(M, k)) return rc;
  DistSide &S = transposed ? M->t : M->a;
  const std::vector<double *> &vx = k > 1 ? M->kw.x : M->x, &vy = k > 1 ? M->kw.y : M->y, &vz = k > 1 ? M->kw.z : M->z;
  // (u of z = A' u lives where y does: A then A' chains without a copy)
  const std::vector<double *> &own_in = transposed ? vy : vx, &own_out = transposed ? vz : vy;
  std::vector<double *> in, out;
  int direct = -1;
  if (int rc = vec_in(M, own_in, x, (size_t)S.ncol * k, in, true)) return rc;
  if (int rc = vec_out(M, own_out, y, out, &direct)) return rc;
  if (int rc = dist_product(M, transposed, k, in, out)) return rc;
  if (direct < 0)
    if (int rc = vec_store(M, 0, y, own_out[0], (size_t)S.nrow * k)) return rc;
  return dist_sync(M->D);
}

int fs_dist_spmv(fs_dist_matrix_t M, double *y, const double *x)
{
  if (!M || !y || !x) { fs::set_error("fs_dist_spmv: NULL argument"); return FS_ERR_ARG; }
  return dist_apply(M, false, y, x, 1);
}

int fs_dist_spmv_t(fs_dist_matrix_t M, double *z, const double *u)
{
  if (!M || !z || !u) { fs::set_error("fs_dist_spmv_t: NULL argument"); return FS_ERR_ARG; }
  if (!M->t.built) { fs::set_error("fs_dist_spmv_t: call fs_dist_matrix_build_transpose first"); return FS_ERR_NO_TRANSPOSE; }
  return dist_apply(M, true, z, u, 1);
}

// z[ncol] = A'(A x[ncol]) + lambda x (bcsr_AA_mul_B, csr.h:305-319, with lambda = 0; bsbm_AtA, cg.h:9-22, across the GPUs): y = A x
// stays on the devices and is the u of the second product in place; two exchanges and one axpy on the rank that holds the output
int fs_dist_ata(fs_dist_matrix_t M, double *z, const double *x, double lambda)
{
  if (!M || !z || !x) { fs::set_error("fs_dist_ata: NULL argument"); return FS_ERR_ARG; }
  if (!M->t.built) { fs::set_error("fs_dist_ata: call fs_dist_matrix_build_transpose first"); return FS_ERR_NO_TRANSPOSE; }
  std::lock_guard<std::mutex> g(M->lock);
  std::lock_guard<std::mutex> gd(M->D->lock);
  DeviceGuard guard;
  std::vector<double *> in, out;
  int direct = -1;
  if (int rc = vec_in(M, M->x, x, (size_t)M->ncol, in, true)) return rc;
  if (int rc = vec_out(M, M->z, z, out, &direct)) return rc;
  if (int rc = dist_product(M, false, 1, in, M->y)) return rc;
  if (int rc = dist_product(M, true, 1, M->y, out)) return rc;
  if (lambda != 0.0) {
    const int r = direct < 0 ? 0 : direct;
    FS_HIP(hipSetDevice(M->D->dev[r]));
    if (int rc = fs_axpy(M->ncol, lambda, in[(size_t)r], out[(size_t)r], M->D->stream[r])) return rc;
  }
  if (direct < 0)
    if (int rc = vec_store(M, 0, z, M->z[0], (size_t)M->ncol)) return rc;
  return dist_sync(M->D);
}

// device-resident forms: the caller fills fs_dist_x(M, r) on every rank once and iterates -- y = A x, z = A' y, and (square
// matrices) fs_dist_swap_xy to make y the next x -- without anything crossing PCIe; each call returns after every device has
// the whole output vector
int fs_dist_spmv_resident(fs_dist_matrix_t M)
{
  if (!M) { fs::set_error("fs_dist_spmv_resident: NULL handle"); return FS_ERR_ARG; }
  std::lock_guard<std::mutex> g(M->lock);
  std::lock_guard<std::mutex> gd(M->D->lock);
  DeviceGuard guard;
  if (int rc = dist_product(M, false, 1, M->x, M->y)) return rc;
  return dist_sync(M->D);
}

int fs_dist_spmv_t_resident(fs_dist_matrix_t M)
{
  if (!M) { fs::set_error("fs_dist_spmv_t_resident: NULL handle"); return FS_ERR_ARG; }
  if (!M->t.built) { fs::set_error("fs_dist_spmv_t_resident: call fs_dist_matrix_build_transpose first"); return FS_ERR_NO_TRANSPOSE; }
  std::lock_guard<std::mutex> g(M->lock);
  std::lock_guard<std::mutex> gd(M->D->lock);
  DeviceGuard guard;
  if (int rc = dist_product(M, true, 1, M->y, M->z)) return rc;
  return dist_sync(M->D);
}

int fs_dist_swap_xy(fs_dist_matrix_t M)
{
  if (!M) { fs::set_error("fs_dist_swap_xy: NULL handle"); return FS_ERR_ARG; }
  if (M->nrow != M->ncol) { fs::set_error("fs_dist_swap_xy: the matrix is not square"); return FS_ERR_ARG; }
  std::lock_guard<std::mutex> g(M->lock);
  M->x.swap(M->y);
  return FS_OK;
}

// ---- the CG solvers on the row-sharded matrix: fs_dist_cg, fs_dist_pcg, fs_dist_pcgn, fs_dist_pcgn_lambdas, fs_dist_mscg, fs_dist_mscgn,
// fs_dist_cg2 ----
// Everything of a solve is resident and the scalars of the iteration live on the devices (fs_cg.hip's launchers); per iteration
// y = A p and q = A' y.  EVERY rank decides convergence for itself and the host compares the flags of all of them one iteration
// behind: a disagreement (which identical arithmetic rules out, and a faulty device or exchange does not) is an error return,
// never a rank waiting in a collective for one that left.  Products run with fixed-order sums unless option "cg_fixed_order" is
// 0.  Work vectors are kept on the handle between solves.  A solve CLOBBERS fs_dist_x / fs_dist_y / fs_dist_z of the handle and
// writes the caller's x once, at the end: whatever fails before leaves it as it was.
//
// DistSolve is the host frame the seven share, the counterpart of CgSolve in fs_cg.hip: open() (the transpose is there, both
// locks, the caller's device kept, fixed-order products, one set of host-visible flags per rank), slices() (the scheme: what
// lo(), rows(), longest(), shard_product(), take_slices() and store() answer with), stage() (the caller's vectors onto the
// ranks), iterate() and finish() (settle(): the agreed final state; agree(): whatever else the solver's ranks must have in
// common; then store(): X to the caller).  A solver brings its argument checks, its work space (st: every rank's st[]; dinv:
// every rank's inverse diagonal, where it has a preconditioner), its start and what an iteration enqueues.
enum { kRanksGoOn = 0, kRanksStopped = 1, kRanksDisagree = 2 };

// T = A P, then Q = A' T: the pair of sharded k-column products (k = 1: the single-vector ones) every solver is built on
static int dist_pair(fs_dist_matrix_t M, int k, const std::vector<double *> &p, const std::vector<double *> &t, const std::vector<double *> &q)
{
  if (int rc = dist_product(M, false, k, p, t)) return rc;
  return dist_product(M, true, k, t, q);
}

// the product vectors of the handle for k columns (x / y / z, or KWork's for k > 1, which ensure_k made): P (replicated input of
// A), T = A P, Q = A' T
struct ProductVectors { const std::vector<double *> &p, &t, &q; };
static ProductVectors product_vectors(fs_dist_matrix_t M, int k)
{
  return k > 1 ? ProductVectors{M->kw.x, M->kw.y, M->kw.z} : ProductVectors{M->x, M->y, M->z};
}

// What a solver's ranks must have in common at the end beside {done, iterations}: on every rank d, count doubles at on[d] + at
struct Outcome { const std::vector<double *> &on; size_t at, count; };
struct Agreement {
  std::vector<Outcome> what;                                   // fetched one behind the other into one host array per rank
  std::function<bool(const double *, const double *)> same;    // (rank d's array, rank 0's)
  const char *differ;                                          // the error text
  std::vector<double> first;                                   // afterwards: rank 0's array, which speaks for all
};

struct DistSolve {
  const char *who;
  fs_dist_matrix_t M;
  fs_dist_t D = M->D;
  const int n = D->n, F = M->ncol;
  std::unique_lock<std::mutex> matrix_lock{M->lock, std::defer_lock}, context_lock{D->lock, std::defer_lock};
  DeviceGuard guard;
  fs::FixedOrderScope fixed{fs::options().cg_fixed_order != 0};
  std::vector<fs::CgFlags> fl = std::vector<fs::CgFlags>((size_t)n);
  const std::vector<double *> *st = nullptr, *dinv = nullptr;
  bool sliced = false;
  int staged = 0;
  int seen = kRanksGoOn;                                   // what the ranks' flags said last: go on, all stopped, or only some did
  int iterations = 0;                                      // after finish(): the agreed count, and rank 0's final st[]
  double st0[fs::kCgStateDoubles];

  int open(const char *no_transpose)
  {
    if (!M->t.built) { fs::set_error(std::string(who) + ": " + no_transpose); return FS_ERR_NO_TRANSPOSE; }
    matrix_lock.lock();
    context_lock.lock();
    return each_rank(D, false, [&](int d) { return fl[(size_t)d].init(); });
  }
  // The scheme: a rank works on whole vectors (rows [0, F) on every rank), or (scheme "gather") on its slice -- the rows of A' it
  // owns.  longest(): of the vectors a rank keeps, at least 1
  void slices(bool gather) { sliced = gather; }
  int lo(int d) const { return sliced ? M->t.bounds[(size_t)d] : 0; }
  int rows(int d) const { return sliced ? M->t.bounds[(size_t)d + 1] - M->t.bounds[(size_t)d] : F; }
  int longest() const
  {
    int longest = 1;
    for (int d = 0; d < n; ++d) longest = std::max(longest, rows(d));
    return longest;
  }
  const double *dinv_of(int d) const { return dinv ? (*dinv)[(size_t)d] : nullptr; }
  // q_r = A'_r t on rank d (slices): the rank's own shard product, no exchange; an empty slice has none
  int shard_product(int d, int k, double *q, const double *t)
  {
    if (rows(d) <= 0) return FS_OK;
    return k == 1 ? fs_spmv(M->t.shard[(size_t)d], q, t, D->stream[d]) : fs_spmm(M->t.shard[(size_t)d], q, t, k, D->stream[d]);
  }
  // every rank's slice of a whole k-column panel that was staged in `whole`
  int take_slices(const std::vector<double *> &dst, const std::vector<double *> &whole, int k)
  {
    return each_rank(D, false, [&](int d) -> int {
      if (rows(d) > 0)
        FS_HIP(hipMemcpyAsync(dst[(size_t)d], whole[(size_t)d] + (size_t)lo(d) * k, sizeof(double) * (size_t)rows(d) * k,
                              hipMemcpyDeviceToDevice, D->stream[d]));
      return FS_OK;
    });
  }
  // `count` doubles of the caller's (host memory or HBM) into own[r] on every rank: always a copy, they are read all solve long.
  // A second and third vector of one call wait for the uploads of the one before, which still read the pinned staging buffer
  int stage(const std::vector<double *> &own, const double *src, size_t count)
  {
    std::vector<double *> unused;
    if (staged++)
      if (int rc = dist_sync(D)) return rc;
    return vec_in(M, own, src, count, unused, false);
  }
  // all ranks said the same (the answer is in `seen`), or only `stops` of them did
  void agreed(int stops, const char *when)
  {
    seen = stops == 0 ? kRanksGoOn : stops == n ? kRanksStopped : kRanksDisagree;
    if (seen == kRanksDisagree) fs::set_error(std::string(who) + ": the devices disagree about convergence" + when);
  }
  // a solve that may be done before its first iteration (b = 0, a warm start from a converged x): one synchronous look at every
  // rank's flag
  int look()
  {
    if (int rc = dist_sync(D)) return rc;
    int stops = 0;
    if (int rc = each_rank(D, false, [&](int d) -> int {
          double done = 0.0;
          FS_HIP(hipMemcpy(&done, (*st)[(size_t)d] + fs::kCgStateDone, sizeof(double), hipMemcpyDeviceToHost));
          stops += done != 0.0 ? 1 : 0;
          return FS_OK;
        })) return rc;
    agreed(stops, " at the start");
    return FS_OK;
  }
  // up to cap iterations, as long as the ranks go on: products() (whatever spans the ranks), then rank by rank in one pass
  // steps(d) (none on slices: their steps span the ranks), the rank's flags on their way to the host and a look at those of the
  // iteration before.  look_first: see look()
  int iterate(int cap, bool look_first, const std::function<int()> &products, const std::function<int(int)> &steps = nullptr)
  {
    if (look_first)
      if (int rc = look()) return rc;
    for (int iter = 0; seen == kRanksGoOn && iter < cap; iter++) {
      if (int rc = products()) return rc;
      int stops = 0;
      if (int rc = each_rank(D, false, [&](int d) -> int {
            bool stop = false;
            if (steps)
              if (int rc2 = steps(d)) return rc2;
            if (int rc2 = fl[(size_t)d].after_iteration(iter, (*st)[(size_t)d], D->stream[d], &stop)) return rc2;
            stops += stop ? 1 : 0;
            return FS_OK;
          })) return rc;
      agreed(stops, " (a device or an exchange returned different bits)");
    }
    return FS_OK;
  }
  // every rank's final {done, iterations} must agree as well; rank 0's final st[] is kept for fs_debug_last_cg_state
  int settle()
  {
    if (int rc = dist_sync(D)) return rc;
    if (seen == kRanksDisagree) return FS_ERR_HIP;
    double fin0[2] = {0.0, 0.0};
    if (int rc = each_rank(D, false, [&](int d) -> int {
          double fin[2];
          FS_HIP(hipMemcpy(fin, (*st)[(size_t)d] + fs::kCgStateDone, sizeof(fin), hipMemcpyDeviceToHost));
          if (d == 0) { fin0[0] = fin[0]; fin0[1] = fin[1]; }
          if (fin[0] != fin0[0] || fin[1] != fin0[1]) {
            fs::set_error(std::string(who) + ": the devices finished in different states");
            return FS_ERR_HIP;
          }
          return FS_OK;
        })) return rc;
    FS_HIP(hipSetDevice(D->dev[0]));
    FS_HIP(hipMemcpy(st0, (*st)[0], sizeof(st0), hipMemcpyDeviceToHost));
    fs::note_cg_state(st0);
    iterations = (int)fin0[1];
    return FS_OK;
  }
  // every rank's array of outcomes against rank 0's
  int agree(Agreement &a)
  {
    std::vector<double> other;
    return each_rank(D, false, [&](int d) -> int {
      std::vector<double> &mine = d == 0 ? a.first : other;
      mine.clear();
      for (const Outcome &o : a.what) {
        mine.resize(mine.size() + o.count);
        FS_HIP(hipMemcpy(mine.data() + mine.size() - o.count, o.on[(size_t)d] + o.at, sizeof(double) * o.count, hipMemcpyDeviceToHost));
      }
      if (d > 0 && !a.same(other.data(), a.first.data())) { fs::set_error(a.differ); return FS_ERR_HIP; }
      return FS_OK;
    });
  }
  // m vectors of k columns to the caller, asynchronously, ld doubles apart on the rank and ldx at the caller: whole from rank 0, or
  // (slices) every rank's rows of A' from its own
  int store(double *x, const std::vector<double *> &sol, int k, int m, size_t ld, size_t ldx)
  {
    for (int i = 0; i < m; ++i)
      for (int d = 0; d < (sliced ? n : 1); ++d)
        if (rows(d) > 0)
          if (int rc = vec_store(M, d, x + (size_t)i * ldx + (size_t)lo(d) * k, sol[(size_t)d] + (size_t)i * ld, (size_t)rows(d) * k)) return rc;
    return FS_OK;
  }
  // The end of a solve: the agreed final state; what else the solver wants agreed; then, and only then, X to the caller
  int finish(double *x, const std::vector<double *> &sol, int k = 1, Agreement *also = nullptr, int m = 1, size_t ld = 0, size_t ldx = 0)
  {
    if (int rc = settle()) return rc;
    if (also)
      if (int rc = agree(*also)) return rc;
    if (vector_device(x) >= 0)
      if (int rc = wait_for_caller(vector_device(x))) return rc;
    if (int rc = store(x, sol, k, m, ld, ldx)) return rc;
    return dist_sync(D);
  }
};

// fs_dist_cg's and fs_dist_pcg's vectors on the handle: whole vectors (scheme "replicate") or slices (scheme "gather") of F doubles
// with room for a slice to be sent as a window of max_rows doubles
static int ensure_cg_work(fs_dist_matrix_t M)
{
  fs_dist_t D = M->D;
  const int n = D->n, F = M->ncol;
  CgWork &W = M->cg;
  if (W.mem.ready && W.F == F) return FS_OK;
  free_work(D, W);
  W.F = F;
  const size_t fl = (size_t)(F ? F : 1) + (size_t)M->t.plan.max_rows + 1;
  return W.mem.fill(D, [&](int d) -> int {
    for (std::vector<double *> *v : {&W.sol, &W.r, &W.b, &W.p, &W.q, &W.dinv})
      if (int rc2 = W.mem.get(d, *v, fl)) return rc2;
    if (int rc2 = W.mem.get(d, W.part, (size_t)fs::kCgPartDoubles)) return rc2;
    if (int rc2 = W.mem.get(d, W.red, (size_t)(3 * kCgSendDoubles))) return rc2;
    if (int rc2 = W.mem.get(d, W.redall, (size_t)(kCgSendDoubles * n + 1))) return rc2;
    return W.mem.get(d, W.st, (size_t)fs::kCgStateDoubles);
  });
}

// Scheme "gather": the sums over the ranks.  A partial reduction leaves a rank's nv sums (1, or 2 that fs_pcg takes in one pass)
// in send(d); combine() all-gathers them, `count` doubles per rank (nv, or ns per column of a k-column solver: ns * k), and every
// rank takes its scalar step over the gathered values, which adds each sum over the ranks in rank order (stage 2's tree).  The
// two send slots, `stride` doubles apart in slots[d], alternate: a rank may be one exchange ahead of another that still reads its
// previous partial.  The one exchange of sums of every solver: CgWork's (red, redall) or PnWork's (send, all) buffers
struct SliceSums {
  fs_dist_matrix_t M;
  const std::vector<double *> &slots, &all;
  int stride;
  int slot = 0;
  double *send(int d) const { return slots[(size_t)d] + stride * slot; }
  // step(d, the gathered values on rank d, rank-major): the scalar step of rank d
  int combine(size_t count, const std::function<int(int, const double *)> &step)
  {
    fs_dist_t D = M->D;
    DistSide &T = M->t;
    std::vector<const double *> from((size_t)D->n);
    std::vector<hipEvent_t> ready((size_t)D->n);
    if (int rc = each_rank(D, false, [&](int d) -> int {
          from[(size_t)d] = send(d);
          FS_HIP(hipEventRecord(T.ev[(size_t)d][0], D->stream[d]));
          ready[(size_t)d] = T.ev[(size_t)d][0];
          return FS_OK;
        })) return rc;
    if (int rc = exchange_equal(D, from, all, count, D->stream, ready)) return rc;
    if (int rc = each_rank(D, false, [&](int d) { return step(d, all[(size_t)d]); })) return rc;
    slot ^= 1;
    return FS_OK;
  }
};

// CgWork's sums (fs_dist_cg, fs_dist_pcg, fs_dist_mscg): where rank d's launchers leave theirs -- in `send`, the rank's send slot
// (scheme "gather"), or finished (nullptr: whole vectors) -- and where the scalar step behind an exchange leaves the finished
// sums: behind the two slots
static fs::CgSums cg_sums(const CgWork &W, int d, double *send)
{
  return fs::CgSums{W.part[(size_t)d], W.red[(size_t)d], W.st[(size_t)d], send};
}
static double *cg_finished_sums(const CgWork &W, int d) { return W.red[(size_t)d] + 2 * kCgSendDoubles; }
static int cg_combine(SliceSums &sums, fs::CgStep step, double arg, int nv)
{
  fs_dist_matrix_t M = sums.M;
  return sums.combine((size_t)nv, [&](int d, const double *all) {
    return fs::cg_dev_final(step, all, M->D->n, cg_finished_sums(M->cg, d), M->cg.st[(size_t)d], arg, M->D->stream[d], nv);
  });
}
// PnWork's sums (the k-column solvers)
static fs::PcgnSums pn_sums(const PnWork &W, int d, double *send)
{
  return fs::PcgnSums{W.part[(size_t)d], W.st[(size_t)d], W.cs[(size_t)d], send};
}

// the iterations of fs_dist_cg and fs_dist_pcg, which differ in the preconditioner (f.dinv: rank d's is cg.dinv[d]) and in the
// convergence step `beta`.  Scheme "replicate": both products carry their all-gather, every rank runs the whole-vector steps.
// Scheme "gather": q_r = A'_r y is the rank's own rows of A', no exchange; the slice steps with their sums combined over the
// ranks; the new p slice all-gathered for the next product
static int cg_iterations(DistSolve &f, SliceSums &sums, int cap, double lambda, fs::CgStep beta)
{
  fs_dist_matrix_t M = f.M;
  fs_dist_t D = f.D;
  CgWork &W = M->cg;
  if (!f.sliced)
    return f.iterate(cap, false, [&] { return dist_pair(M, 1, M->x, M->y, M->z); }, [&](int d) {      // y = A p, q = A' y
      return fs::cg_dev_steps(f.F, lambda, W.sol[(size_t)d], W.r[(size_t)d], M->x[(size_t)d], M->z[(size_t)d], f.dinv_of(d),
                              cg_sums(W, d, nullptr), beta, D->stream[d]);
    });
  return f.iterate(cap, false, [&]() -> int {
    if (int rc = dist_product(M, false, 1, M->x, M->y)) return rc;         // y = A p
    if (int rc = each_rank(D, false, [&](int d) -> int {
          if (int rc2 = f.shard_product(d, 1, W.q[(size_t)d], M->y[(size_t)d])) return rc2;
          return fs::cg_dev_shift_dot(f.rows(d), lambda, W.p[(size_t)d], W.q[(size_t)d], cg_sums(W, d, sums.send(d)), D->stream[d]);
        })) return rc;
    if (int rc = cg_combine(sums, fs::kStepCgAlpha, 0.0, 1)) return rc;    // alpha
    if (int rc = each_rank(D, false, [&](int d) {
          return fs::cg_dev_update(f.rows(d), W.sol[(size_t)d], W.r[(size_t)d], W.p[(size_t)d], W.q[(size_t)d], f.dinv_of(d),
                                   cg_sums(W, d, sums.send(d)), beta, D->stream[d]);
        })) return rc;
    if (int rc = cg_combine(sums, beta, 0.0, f.dinv ? 2 : 1)) return rc;   // converged?  beta
    if (int rc = each_rank(D, false, [&](int d) {
          return fs::cg_dev_direction(f.rows(d), W.p[(size_t)d], W.r[(size_t)d], f.dinv_of(d), W.st[(size_t)d], D->stream[d]);
        })) return rc;
    return run_gather(D, exchange_of(M, true, 1), W.p, M->x, false);       // the new p on every rank
  });
}

// (A'A + lambda I) x = b on the row-sharded matrix: bsbm_cg (cg.h:25-82) across the GPUs.  Two schemes for everything but
// y = A p (option "dist_cg_scheme"):
//   0 "replicate"  every device keeps the WHOLE x, r, p, q and runs the same fused vector kernels on them -- identical inputs,
//                  identical kernels, identical vectors: the dots need no exchange.  Both products carry their all-gather.
//                  The O(F) vector work is done N times over.
//   1 "gather"     (libfastsparse_amd/dist.py ShardedCG's scheme) rank r keeps ITS SLICE of x, r, p, q -- the rows of A' it owns.
//                  q_r = A'_r y needs no exchange; the dots are partial: every rank's partial is all-gathered (8 bytes per
//                  rank) and every rank adds the N values in rank order, so all ranks hold identical scalars; the new p slice is
//                  all-gathered (whole-shard exchange) for the next product.  The vector work is divided by N; two tiny
//                  exchanges per iteration are added.
int fs_dist_cg(fs_dist_matrix_t M, double *x_host, const double *b_host, double lambda, double tol, int *out_iter)
{
  if (!M || !x_host || !b_host) { fs::set_error("fs_dist_cg: NULL argument"); return FS_ERR_ARG; }
  DistSolve f{"fs_dist_cg", M};
  if (int rc = f.open("call fs_dist_matrix_build_transpose first")) return rc;
  fs_dist_t D = f.D;
  const int F = f.F;
  const bool gather = fs::options().dist_cg_scheme == 1 && f.n > 1;
  f.slices(gather);
  CgWork &W = M->cg;
  if (int rc = ensure_cg_work(M)) return rc;
  f.st = &W.st;
  if (int rc = f.stage(W.b, b_host, (size_t)F)) return rc;
  SliceSums sums{M, W.red, W.redall, kCgSendDoubles};
  if (int rc = each_rank(D, false, [&](int d) {                          // cg_init_kernel writes p itself: whole into x, or the slice
        return fs::cg_dev_init(f.rows(d), W.b[(size_t)d] + f.lo(d), W.sol[(size_t)d], W.r[(size_t)d], (gather ? W.p : M->x)[(size_t)d],
                               cg_sums(W, d, gather ? sums.send(d) : nullptr), tol, D->stream[d]);
      })) return rc;
  if (gather) {
    if (int rc = cg_combine(sums, fs::kStepCgStart, tol, 1)) return rc;
    if (int rc = run_gather(D, exchange_of(M, true, 1), W.p, M->x, false)) return rc;     // the whole p on every rank
  }
  if (int rc = cg_iterations(f, sums, F, lambda, fs::kStepCgBeta)) return rc;
  if (int rc = f.finish(x_host, W.sol)) return rc;
  if (out_iter) *out_iter = f.iterations;
  return FS_OK;
}

// ---- the preconditioned solvers on the row-sharded matrix: fs_gram_diag, fs_pcg, fs_pcgn across the ranks ------------------
// Jacobi reads the plain CSR of every rank's shard of A': FS_ERR_RELEASED before anything else happens
static int gram_diag_ready(fs_dist_matrix_t M, const char *who)
{
  DistSide &T = M->t;
  for (int r = 0; r < M->D->n; ++r)
    if (T.bounds[(size_t)r + 1] > T.bounds[(size_t)r])
      if (int rc = fs::need_plain_csr(T.shard[(size_t)r]->a, who)) return rc;
  return FS_OK;
}

// rank r: gram_diag_kernel over the rows of A' it owns, into dst[r] (slice-local)
static int gram_diag_slices(fs_dist_matrix_t M, double lambda, const std::vector<double *> &dst)
{
  DistSide &T = M->t;
  return each_rank(M->D, false, [&](int r) -> int {
    if (T.bounds[(size_t)r + 1] == T.bounds[(size_t)r]) return FS_OK;
    return fs_gram_diag(T.shard[(size_t)r], lambda, dst[(size_t)r], M->D->stream[r]);
  });
}

// the whole d on every rank, in out[r]: the slices into the side's local buffers, then one whole-shard gather
static int gram_diag_everywhere(fs_dist_matrix_t M, double lambda, const std::vector<double *> &out)
{
  if (int rc = context_usable(M->D)) return rc;
  if (int rc = gram_diag_slices(M, lambda, M->t.local)) return rc;
  return run_gather(M->D, exchange_of(M, true, 1), M->t.local, out, false);
}

// d = the diagonal of A'A + lambda I: fs_gram_diag on every rank's rows of A'.  CLOBBERS fs_dist_z (unless d itself is in HBM
// of a rank's device: then the gather writes it)
int fs_dist_gram_diag(fs_dist_matrix_t M, double lambda, double *d)
{
  if (!M || !d) { fs::set_error("fs_dist_gram_diag: NULL argument"); return FS_ERR_ARG; }
  if (!M->t.built) { fs::set_error("fs_dist_gram_diag: call fs_dist_matrix_build_transpose first"); return FS_ERR_NO_TRANSPOSE; }
  std::lock_guard<std::mutex> g(M->lock);
  std::lock_guard<std::mutex> gd(M->D->lock);
  DeviceGuard guard;
  if (int rc = gram_diag_ready(M, "fs_dist_gram_diag")) return rc;
  std::vector<double *> out;
  int direct = -1;
  if (int rc = vec_out(M, M->z, d, out, &direct)) return rc;
  if (int rc = gram_diag_everywhere(M, lambda, out)) return rc;
  if (direct < 0)
    if (int rc = vec_store(M, 0, d, M->z[0], (size_t)M->ncol)) return rc;
  return dist_sync(M->D);
}

// fs_pcg across the ranks; the schemes are fs_dist_cg's (option "dist_cg_scheme"), and so are the iterations (cg_iterations):
//   0 "replicate"  every rank holds whole x, r, p, q, dinv and launches fs_pcg's own kernels on them: no exchange for the sums.
//                  Jacobi costs one gather of d per solve, a warm start one pair of sharded products on x0.
//   1 "gather"     rank r keeps its slice -- the rows of A' it owns -- of x, r, p, q, dinv.  Jacobi's slice of d is the rank's own
//                  gram_diag launch: no exchange.  Every sum is the slice tree of fs_dist_cg (SliceSums); the sums fs_pcg takes in one
//                  pass travel together: {b.b, r.r} at the start, {r.r, r.z} behind the update with a preconditioner.
int fs_dist_pcg(fs_dist_matrix_t M, double *x, const double *b, double lambda, const fs_pcg_params *prm, fs_pcg_info *info)
{
  if (!M || !x || !b || !prm) { fs::set_error("fs_dist_pcg: NULL argument"); return FS_ERR_ARG; }
  if (int rc = fs::pcg_params_ok("fs_dist_pcg", prm)) return rc;
  DistSolve f{"fs_dist_pcg", M};
  if (int rc = f.open("call fs_dist_matrix_build_transpose first")) return rc;
  if (prm->precond == FS_PRECOND_JACOBI)
    if (int rc = gram_diag_ready(M, "fs_dist_pcg with FS_PRECOND_JACOBI (fs_gram_diag)")) return rc;
  fs_dist_t D = f.D;
  const int F = f.F;
  const bool gather = fs::options().dist_cg_scheme == 1 && f.n > 1;
  const bool pre = prm->precond != FS_PRECOND_NONE, warm = prm->warm_start != 0;
  const int cap = prm->max_iter > 0 ? prm->max_iter : F;     // cg.h:55
  f.slices(gather);
  CgWork &W = M->cg;
  if (int rc = ensure_cg_work(M)) return rc;
  f.st = &W.st;
  f.dinv = pre ? &W.dinv : nullptr;
  // a rank works on whole vectors or on its slice; q and p are the handle's z and x (whole) or the rank's slice buffers, and d is
  // staged in the vector that holds q later
  const std::vector<double *> &vq = gather ? W.q : M->z, &vp = gather ? W.p : M->x;
  if (int rc = f.stage(W.b, b, (size_t)F)) return rc;
  if (warm)                                                                      // x0, whole, on every rank
    if (int rc = f.stage(gather ? M->x : W.sol, x, (size_t)F)) return rc;
  if (prm->precond == FS_PRECOND_DIAG)
    if (int rc = f.stage(vq, prm->diag, (size_t)F)) return rc;
  SliceSums sums{M, W.red, W.redall, kCgSendDoubles};
  if (prm->precond == FS_PRECOND_JACOBI)                                         // whole: one gather of d; else the rank's own rows
    if (int rc = gather ? gram_diag_slices(M, lambda, vq) : gram_diag_everywhere(M, lambda, vq)) return rc;
  if (pre)
    if (int rc = each_rank(D, false, [&](int d) {                               // (a staged d is whole, Jacobi's is the slice)
          const double *dd = vq[(size_t)d] + (prm->precond == FS_PRECOND_DIAG ? f.lo(d) : 0);
          return fs::pcg_dev_dinv(f.rows(d), dd, W.dinv[(size_t)d], D->stream[d]);
        })) return rc;
  if (warm && !gather)                                                           // q = A'(A x0)
    if (int rc = dist_pair(M, 1, W.sol, M->y, M->z)) return rc;
  if (warm && gather) {                                                          // the rank's slice of x0; q_r = A'_r (A x0)
    if (int rc = f.take_slices(W.sol, M->x, 1)) return rc;
    if (int rc = dist_product(M, false, 1, M->x, M->y)) return rc;
    if (int rc = each_rank(D, false, [&](int d) { return f.shard_product(d, 1, W.q[(size_t)d], M->y[(size_t)d]); })) return rc;
  }
  // b.b, r.r, stop, done?  then p = z, r.z.  Whole vectors: a rank's two steps in one pass; slices: each with its sums combined
  if (int rc = each_rank(D, false, [&](int d) -> int {
        if (int rc2 = fs::pcg_dev_init(f.rows(d), warm, lambda, W.b[(size_t)d] + f.lo(d), W.sol[(size_t)d], W.r[(size_t)d], vq[(size_t)d],
                                       cg_sums(W, d, gather ? sums.send(d) : nullptr), prm->tol, D->stream[d])) return rc2;
        return gather ? FS_OK : fs::pcg_dev_start(F, W.r[(size_t)d], f.dinv_of(d), vp[(size_t)d], cg_sums(W, d, nullptr), D->stream[d]);
      })) return rc;
  if (gather) {
    if (int rc = cg_combine(sums, fs::kStepPcgStart, prm->tol, 2)) return rc;
    if (int rc = each_rank(D, false, [&](int d) {
          return fs::pcg_dev_start(f.rows(d), W.r[(size_t)d], f.dinv_of(d), vp[(size_t)d], cg_sums(W, d, sums.send(d)), D->stream[d]);
        })) return rc;
    if (int rc = cg_combine(sums, fs::kStepPcgRz, 0.0, 1)) return rc;
  }
  if (int rc = f.look()) return rc;                          // done before the first iteration: no product is enqueued
  if (gather && f.seen == kRanksGoOn)
    if (int rc = run_gather(D, exchange_of(M, true, 1), W.p, M->x, false)) return rc;     // the whole p on every rank
  if (int rc = cg_iterations(f, sums, cap, lambda, fs::kStepPcgBeta)) return rc;
  if (int rc = f.finish(x, W.sol)) return rc;
  fs::pcg_info_of(f.st0, info);
  return FS_OK;
}

// the k-column solvers' vectors on the handle: whole F x k panels on every rank, or (slices) the rank's rows of A' of them with the
// send slots and the gathered sums.  Kept between solves; re-made when k or the scheme changes
static int ensure_pn_work(fs_dist_matrix_t M, int k, bool slices)
{
  fs_dist_t D = M->D;
  const int n = D->n, F = M->ncol;
  PnWork &W = M->pn;
  if (W.mem.ready && W.F == F && W.k == k && W.slices == slices) return FS_OK;
  if (int rc = dist_sync(D)) return rc;
  free_work(D, W);
  W.F = F; W.k = k; W.slices = slices;
  return W.mem.fill(D, [&](int d) -> int {
    const size_t rows = slices ? (size_t)(M->t.bounds[(size_t)d + 1] - M->t.bounds[(size_t)d]) : (size_t)F;
    const size_t fk = (rows ? rows : 1) * (size_t)k;
    for (std::vector<double *> *v : {&W.sol, &W.r, &W.b})
      if (int rc2 = W.mem.get(d, *v, fk)) return rc2;
    if (int rc2 = W.mem.get(d, W.dinv, rows ? rows : 1)) return rc2;
    if (int rc2 = W.mem.get(d, W.part, fs::pcgn_part_doubles(k))) return rc2;
    if (int rc2 = W.mem.get(d, W.cs, (size_t)fs::kPcgnStateDoubles)) return rc2;
    if (slices) {
      if (int rc2 = W.mem.get(d, W.q, fk)) return rc2;
      if (int rc2 = W.mem.get(d, W.send, (size_t)(2 * fs::kPcgnSendDoubles))) return rc2;
      if (int rc2 = W.mem.get(d, W.all, (size_t)n * fs::kPcgnSendDoubles)) return rc2;
    }
    return W.mem.get(d, W.st, (size_t)fs::kCgStateDoubles);
  });
}

// The replicated k-column frame of fs_dist_pcgn and of scheme 0 of fs_dist_pcgn_lambdas, from staging to the last iteration: every
// rank holds the whole F x k panels (PnWork; ensure_k and ensure_pn_work are done) and launches the solver's own instantiations
// of fs_pcgn's kernels on them -- init(d), then steps(d) behind every pair of sharded k-column products.  fill_dinv(): what the
// solver enqueues between staging and the warm start's products -- its diagonal (a caller's d is staged in Q's vector) into dinv
static int pcgn_replicated(DistSolve &f, double *X, const double *B, int k, const fs_pcg_params *prm, const std::function<int()> &fill_dinv,
                           const std::function<int(int)> &init, const std::function<int(int)> &steps)
{
  fs_dist_matrix_t M = f.M;
  PnWork &W = M->pn;
  const size_t F = (size_t)f.F;
  const ProductVectors v = product_vectors(M, k);
  if (int rc = f.stage(W.b, B, F * k)) return rc;
  if (prm->warm_start)
    if (int rc = f.stage(W.sol, X, F * k)) return rc;
  if (prm->precond == FS_PRECOND_DIAG)
    if (int rc = f.stage(v.q, prm->diag, F)) return rc;                            // (d is staged where Q lives later)
  if (int rc = fill_dinv()) return rc;
  if (prm->warm_start)                                       // Q = A'(A X0): one pair of k-column products
    if (int rc = dist_pair(M, k, W.sol, v.t, v.q)) return rc;
  if (int rc = each_rank(f.D, false, init)) return rc;
  return f.iterate(prm->max_iter > 0 ? prm->max_iter : f.F /* cg.h:55 */, true, [&] { return dist_pair(M, k, v.p, v.t, v.q); }, steps);
}

// fs_pcgn across the ranks, replicated whatever "dist_cg_scheme" says: every rank holds the whole F x k panels and launches
// fs_pcgn's own kernels on them (pcgn_dev_*); T = A P and Q = A' T are the sharded k-column products (k = 1: the single-vector
// ones).
int fs_dist_pcgn(fs_dist_matrix_t M, double *X, const double *B, int k, double lambda, const fs_pcg_params *prm, fs_pcg_info *info)
{
  if (!M || !X || !B || !prm) { fs::set_error("fs_dist_pcgn: NULL argument"); return FS_ERR_ARG; }
  if (k < 1 || k > FS_PCGN_MAX_RHS) { fs::set_error("fs_dist_pcgn: k outside 1..FS_PCGN_MAX_RHS"); return FS_ERR_ARG; }
  if (int rc = fs::pcg_params_ok("fs_dist_pcgn", prm)) return rc;
  DistSolve f{"fs_dist_pcgn", M};
  if (int rc = f.open("call fs_dist_matrix_build_transpose first")) return rc;
  if (prm->precond == FS_PRECOND_JACOBI)
    if (int rc = gram_diag_ready(M, "fs_dist_pcgn with FS_PRECOND_JACOBI (fs_gram_diag)")) return rc;
  fs_dist_t D = f.D;
  const int F = f.F;
  const bool pre = prm->precond != FS_PRECOND_NONE, warm = prm->warm_start != 0;
  if (k > 1)
    if (int rc = ensure_k(M, k)) return rc;
  PnWork &W = M->pn;
  if (int rc = ensure_pn_work(M, k, false)) return rc;
  f.st = &W.st;
  f.dinv = pre ? &W.dinv : nullptr;
  const ProductVectors v = product_vectors(M, k);
  // the column state cleared; Jacobi at lambda goes where a caller's d is staged, and either through the inverse pass
  if (int rc = pcgn_replicated(f, X, B, k, prm, [&]() -> int {
        if (int rc2 = each_rank(D, false, [&](int d) { return fs::pcgn_dev_clear(W.cs[(size_t)d], D->stream[d]); })) return rc2;
        if (prm->precond == FS_PRECOND_JACOBI)
          if (int rc2 = gram_diag_everywhere(M, lambda, v.q)) return rc2;
        if (!pre) return FS_OK;
        return each_rank(D, false, [&](int d) { return fs::pcg_dev_dinv(F, v.q[(size_t)d], W.dinv[(size_t)d], D->stream[d]); });
      }, [&](int d) {
        return fs::pcgn_dev_init(F, k, warm, lambda, W.b[(size_t)d], W.sol[(size_t)d], W.r[(size_t)d], v.p[(size_t)d], v.q[(size_t)d],
                                 f.dinv_of(d), W.part[(size_t)d], W.st[(size_t)d], W.cs[(size_t)d], prm->tol, D->stream[d]);
      }, [&](int d) {
        return fs::pcgn_dev_steps(F, k, lambda, W.sol[(size_t)d], W.b[(size_t)d], W.r[(size_t)d], v.p[(size_t)d], v.q[(size_t)d],
                                  f.dinv_of(d), W.part[(size_t)d], W.st[(size_t)d], W.cs[(size_t)d], D->stream[d]);
      })) return rc;
  if (int rc = f.finish(X, W.sol, k)) return rc;
  double cs0[fs::kPcgnStateDoubles] = {0.0};
  FS_HIP(hipSetDevice(D->dev[0]));
  FS_HIP(hipMemcpy(cs0, W.cs[0], sizeof(double) * (size_t)k * (fs::kPcgnStateDoubles / FS_PCGN_MAX_RHS), hipMemcpyDeviceToHost));
  fs::pcgn_note_state(f.st0, cs0, k, info);
  return FS_OK;
}

// fs_pcgn_lambdas across the ranks; the schemes are fs_dist_pcg's (option "dist_cg_scheme"):
//   0 "replicate"  fs_dist_pcgn's frame (pcgn_replicated) with fs_pcgn_lambdas' instantiations of the kernels on whole panels.
//                  Jacobi: the work vector holds s = fs_gram_diag of A' at 0.0, gathered once; no inverse pass.
//   1 "gather"     rank r keeps its rows of A' of X, R, B, Q and s / dinv; P and T = A P stay whole (the product's input and
//                  output).  Q_r = A'_r T is the rank's own shard product: no exchange.  Every sum is the slice tree of fs_dist_cg
//                  per column: a slice step leaves a rank's ns sums per column in its send slot, SliceSums::combine gathers them,
//                  ns * k doubles per rank, and every rank takes the scalar step of every column over them (pcgn_dev_rank_step).
//                  The new P slices are all-gathered for the next product -- the first P too: it is Z = R dinv, which only the
//                  owner of a row can form.
int fs_dist_pcgn_lambdas(fs_dist_matrix_t M, double *X, const double *B, int k, const double *lambda, const fs_pcg_params *prm,
                         fs_pcg_info *info)
{
  if (!M || !X || !B || !prm || !lambda) { fs::set_error("fs_dist_pcgn_lambdas: NULL argument"); return FS_ERR_ARG; }
  if (k < 1 || k > FS_PCGN_MAX_RHS) { fs::set_error("fs_dist_pcgn_lambdas: k outside 1..FS_PCGN_MAX_RHS"); return FS_ERR_ARG; }
  if (int rc = fs::pcg_params_ok("fs_dist_pcgn_lambdas", prm)) return rc;
  fs::PcgnLambdas lv = {};
  for (int j = 0; j < k; ++j) {
    if (!std::isfinite(lambda[j])) { fs::set_error("fs_dist_pcgn_lambdas: a lambda is NaN or infinite"); return FS_ERR_ARG; }
    lv.v[j] = lambda[j];
  }
  DistSolve f{"fs_dist_pcgn_lambdas", M};
  if (int rc = f.open("call fs_dist_matrix_build_transpose first")) return rc;
  if (prm->precond == FS_PRECOND_JACOBI)
    if (int rc = gram_diag_ready(M, "fs_dist_pcgn_lambdas with FS_PRECOND_JACOBI (fs_gram_diag)")) return rc;
  fs_dist_t D = f.D;
  const int F = f.F, n = f.n;
  const bool gather = fs::options().dist_cg_scheme == 1 && n > 1;
  const bool pre = prm->precond != FS_PRECOND_NONE, warm = prm->warm_start != 0;
  const bool colj = prm->precond == FS_PRECOND_JACOBI;       // the diagonal follows the column: dinv holds s
  const int cap = prm->max_iter > 0 ? prm->max_iter : F;     // cg.h:55
  f.slices(gather);
  if (k > 1)
    if (int rc = ensure_k(M, k)) return rc;
  PnWork &W = M->pn;
  if (int rc = ensure_pn_work(M, k, gather)) return rc;
  f.st = &W.st;
  f.dinv = pre ? &W.dinv : nullptr;
  const ProductVectors v = product_vectors(M, k);              // (Q as a whole panel: scheme 0 only)
  if (int rc = each_rank(D, false, [&](int d) { return fs::pcgn_dev_clear(W.cs[(size_t)d], D->stream[d]); })) return rc;
  if (!gather) {
    // a caller's d through the inverse pass; Jacobi: s at 0.0, as it is
    if (int rc = pcgn_replicated(f, X, B, k, prm, [&]() -> int {
          if (prm->precond == FS_PRECOND_DIAG)
            if (int rc2 = each_rank(D, false, [&](int d) { return fs::pcg_dev_dinv(F, v.q[(size_t)d], W.dinv[(size_t)d], D->stream[d]); })) return rc2;
          return colj ? gram_diag_everywhere(M, 0.0, W.dinv) : FS_OK;
        }, [&](int d) {
          return fs::pcgn_dev_init_lambdas(F, k, warm, lv, colj, W.b[(size_t)d], W.sol[(size_t)d], W.r[(size_t)d], v.p[(size_t)d], v.q[(size_t)d],
                                           f.dinv_of(d), W.part[(size_t)d], W.st[(size_t)d], W.cs[(size_t)d], prm->tol, D->stream[d]);
        }, [&](int d) {
          return fs::pcgn_dev_steps_lambdas(F, k, lv, colj, W.sol[(size_t)d], W.b[(size_t)d], W.r[(size_t)d], v.p[(size_t)d], v.q[(size_t)d],
                                            f.dinv_of(d), W.part[(size_t)d], W.st[(size_t)d], W.cs[(size_t)d], D->stream[d]);
        })) return rc;
  } else {
    // the slice of P: the local output buffer of the A' side, which no product of this scheme writes -- the gather's own source
    const Exchange gp = exchange_of(M, true, k);
    const std::vector<double *> &ps = gp.local;
    SliceSums sums{M, W.send, W.all, fs::kPcgnSendDoubles};
    auto combine = [&](fs::PcgnStep step, int ns, double tol) {
      return sums.combine((size_t)ns * (size_t)k, [&](int d, const double *all) {
        return fs::pcgn_dev_rank_step(step, all, n, k, ns, tol, W.st[(size_t)d], W.cs[(size_t)d], D->stream[d]);
      });
    };
    if (int rc = f.stage(v.p, B, (size_t)F * k)) return rc;                        // whole panels pass through P on their way to the slices
    if (int rc = f.take_slices(W.b, v.p, k)) return rc;
    if (prm->precond == FS_PRECOND_DIAG) {
      if (int rc = f.stage(v.q, prm->diag, (size_t)F)) return rc;                  // (whole, in the product vector this scheme leaves idle)
      if (int rc = each_rank(D, false, [&](int d) {
            return fs::pcg_dev_dinv(f.rows(d), v.q[(size_t)d] + f.lo(d), W.dinv[(size_t)d], D->stream[d]);
          })) return rc;
    }
    if (colj)
      if (int rc = gram_diag_slices(M, 0.0, W.dinv)) return rc;                    // the rank's own rows: no exchange
    if (warm) {                                              // the whole X0 is the product's input; Q_r = A'_r (A X0)
      if (int rc = f.stage(v.p, X, (size_t)F * k)) return rc;
      if (int rc = f.take_slices(W.sol, v.p, k)) return rc;
      if (int rc = dist_product(M, false, k, v.p, v.t)) return rc;
      if (int rc = each_rank(D, false, [&](int d) { return f.shard_product(d, k, W.q[(size_t)d], v.t[(size_t)d]); })) return rc;
    }
    if (int rc = each_rank(D, false, [&](int d) {
          return fs::pcgn_slice_init(f.rows(d), k, warm, lv, W.b[(size_t)d], W.sol[(size_t)d], W.r[(size_t)d], W.q[(size_t)d],
                                     pn_sums(W, d, sums.send(d)), D->stream[d]);
        })) return rc;
    if (int rc = combine(fs::kPnStepStart, 2, prm->tol)) return rc;                // b.b, r.r, stop, live?
    if (int rc = each_rank(D, false, [&](int d) {
          return fs::pcgn_slice_start(f.rows(d), k, lv, colj, W.sol[(size_t)d], W.b[(size_t)d], W.r[(size_t)d], f.dinv_of(d), ps[(size_t)d],
                                      pn_sums(W, d, sums.send(d)), D->stream[d]);
        })) return rc;
    if (int rc = combine(fs::kPnStepRz, 1, 0.0)) return rc;                        // r.z
    if (int rc = f.look()) return rc;                        // done before the first iteration: no product is enqueued
    if (f.seen == kRanksGoOn)
      if (int rc = run_gather(D, gp, ps, v.p, false)) return rc;                   // the whole P on every rank
    if (int rc = f.iterate(cap, false, [&]() -> int {
          if (int rc2 = dist_product(M, false, k, v.p, v.t)) return rc2;           // T = A P
          if (int rc2 = each_rank(D, false, [&](int d) -> int {
                if (int rc3 = f.shard_product(d, k, W.q[(size_t)d], v.t[(size_t)d])) return rc3;
                return fs::pcgn_slice_shift_dot(f.rows(d), k, lv, W.sol[(size_t)d], W.b[(size_t)d], W.q[(size_t)d], ps[(size_t)d],
                                                pn_sums(W, d, sums.send(d)), D->stream[d]);
              })) return rc2;
          if (int rc2 = combine(fs::kPnStepAlpha, 1, 0.0)) return rc2;             // alpha
          if (int rc2 = each_rank(D, false, [&](int d) {
                return fs::pcgn_slice_update(f.rows(d), k, lv, colj, W.sol[(size_t)d], W.b[(size_t)d], W.r[(size_t)d], ps[(size_t)d],
                                             W.q[(size_t)d], f.dinv_of(d), pn_sums(W, d, sums.send(d)), D->stream[d]);
              })) return rc2;
          if (int rc2 = combine(fs::kPnStepBeta, pre ? 2 : 1, 0.0)) return rc2;    // converged?  beta
          if (int rc2 = each_rank(D, false, [&](int d) {
                return fs::pcgn_slice_direction(f.rows(d), k, lv, colj, W.sol[(size_t)d], W.b[(size_t)d], ps[(size_t)d], W.r[(size_t)d],
                                                f.dinv_of(d), pn_sums(W, d, sums.send(d)), D->stream[d]);
              })) return rc2;
          return run_gather(D, gp, ps, v.p, false);                                // the new P on every rank
        })) return rc;
  }
  // every rank froze every column at the same iteration in the same way: the per-column array, then st[] for the live mask
  const size_t ncs = (size_t)k * (fs::kPcgnStateDoubles / FS_PCGN_MAX_RHS);
  Agreement froze{{Outcome{W.cs, 0, ncs}, Outcome{W.st, 0, (size_t)fs::kCgStateDoubles}}, [&](const double *mine, const double *first) {
    return mine[ncs + fs::kCgStateLiveMask] == first[ncs + fs::kCgStateLiveMask] && fs::pcgn_same_outcome(mine, first, k);
  }, "fs_dist_pcgn_lambdas: the devices froze the columns differently (a device or an exchange returned different bits)", {}};
  if (int rc = f.finish(X, W.sol, k, &froze)) return rc;
  fs::pcgn_note_state(f.st0, froze.first.data(), k, info);
  return FS_OK;
}

// A ladder solver's vectors on the handle (W: M->ms or M->mn): room for m x_i and nslots P_i of ld doubles each and `scalars`
// doubles, per rank.  Kept between solves; re-made when a solve needs more vectors or longer ones than they hold
static int ensure_ladder_work(fs_dist_matrix_t M, LadderWork &W, int m, int nslots, long long ld, size_t scalars)
{
  fs_dist_t D = M->D;
  if (W.mem.ready && W.F == M->ncol && W.m >= m && W.nslots >= nslots && W.ld >= ld) return FS_OK;
  if (int rc = dist_sync(D)) return rc;
  free_work(D, W);
  W.F = M->ncol; W.m = m; W.nslots = nslots; W.ld = ld;
  return W.mem.fill(D, [&](int d) -> int {
    if (int rc2 = W.mem.get(d, W.X, (size_t)ld * (size_t)m)) return rc2;
    if (int rc2 = W.mem.get(d, W.P, (size_t)ld * (size_t)(nslots ? nslots : 1))) return rc2;
    return W.mem.get(d, W.sc, scalars);
  });
}

// fs_mscg across the ranks; the schemes are fs_dist_cg's (option "dist_cg_scheme"):
//   0 "replicate"  every rank holds whole r, p, q, the m x_i and the P_i and launches fs_mscg's own kernels on them (mscg_dev_*):
//                  both products carry their all-gather, no exchange for the sums.
//   1 "gather"     rank r keeps its slice -- the rows of A' it owns -- of r, p, q, every x_i and every P_i.  The x_i and P_i never
//                  leave their rank: only p enters a product.  q_r = A'_r y is the rank's own shard; q.p and r.r are the slice tree
//                  of fs_dist_cg (SliceSums), S1 and S2 run on every rank over the N gathered values; the new p is gathered.  The
//                  first p is b, which every rank holds whole after staging.
// The caller's X is written once, at the end, after every rank's {done, iterations} and per-shift {live, converged, count} agreed.
int fs_dist_mscg(fs_dist_matrix_t M, double *X, int64_t ldx, const double *b, int m, const double *lambda, double tol, int max_iter,
                 fs_pcg_info *info)
{
  if (!M || !X || !b || !lambda) { fs::set_error("fs_dist_mscg: NULL argument"); return FS_ERR_ARG; }
  if (int rc = fs::mscg_args_ok("fs_dist_mscg", M->ncol, ldx, m, lambda, tol)) return rc;
  DistSolve f{"fs_dist_mscg", M};
  if (int rc = f.open("call fs_dist_matrix_build_transpose first")) return rc;
  fs_dist_t D = f.D;
  const int F = f.F, n = f.n;
  const bool gather = fs::options().dist_cg_scheme == 1 && n > 1;
  const fs::MscgShifts sh = fs::mscg_shifts(m, lambda);
  const int cap = max_iter > 0 ? max_iter : F;               // cg.h:55
  f.slices(gather);
  if (int rc = ensure_cg_work(M)) return rc;                 // (ld: every x_i and P_i 16-byte aligned)
  if (int rc = ensure_ladder_work(M, M->ms, m, sh.nslots, ((long long)f.longest() + 1) & ~1LL, (size_t)fs::kMscgStateDoubles)) return rc;
  CgWork &W = M->cg;
  LadderWork &S = M->ms;
  const long long ld = S.ld;
  f.st = &W.st;
  // a rank works on whole vectors or on its slice; q and p are the handle's z and x (whole) or the rank's slice buffers
  const std::vector<double *> &vq = gather ? W.q : M->z, &vp = gather ? W.p : M->x;
  auto scalars_of = [&](int d) { return fs::MscgScalars{S.sc[(size_t)d], m, tol, &sh}; };
  if (int rc = f.stage(W.b, b, (size_t)F)) return rc;
  SliceSums sums{M, W.red, W.redall, kCgSendDoubles};
  if (int rc = each_rank(D, false, [&](int d) -> int {       // the init kernel writes p itself: whole into x, or the slice
        if (gather && F > 0)                                 // the first product reads the whole p = b
          FS_HIP(hipMemcpyAsync(M->x[(size_t)d], W.b[(size_t)d], sizeof(double) * (size_t)F, hipMemcpyDeviceToDevice, D->stream[d]));
        return fs::mscg_dev_init(f.rows(d), W.b[(size_t)d] + f.lo(d), W.r[(size_t)d], vp[(size_t)d], S.X[(size_t)d], ld, S.P[(size_t)d], ld,
                                 cg_sums(W, d, gather ? sums.send(d) : nullptr), scalars_of(d), D->stream[d]);
      })) return rc;
  auto combine = [&](fs::MscgStep step) {
    return sums.combine(1, [&](int d, const double *all) {
      return fs::mscg_dev_final(step, all, n, cg_finished_sums(W, d), W.st[(size_t)d], scalars_of(d), D->stream[d]);
    });
  };
  if (gather)
    if (int rc = combine(fs::kMscgStart)) return rc;
  if (!gather) {
    if (int rc = f.iterate(cap, true, [&] { return dist_pair(M, 1, M->x, M->y, M->z); }, [&](int d) {     // y = A p, q = A' y
          return fs::mscg_dev_steps(F, sh.base, W.r[(size_t)d], M->x[(size_t)d], M->z[(size_t)d], S.X[(size_t)d], ld, S.P[(size_t)d], ld,
                                    cg_sums(W, d, nullptr), scalars_of(d), D->stream[d]);
        })) return rc;
  } else {
    if (int rc = f.iterate(cap, true, [&]() -> int {
          if (int rc2 = dist_product(M, false, 1, M->x, M->y)) return rc2;     // y = A p
          if (int rc2 = each_rank(D, false, [&](int d) -> int {
                if (int rc3 = f.shard_product(d, 1, vq[(size_t)d], M->y[(size_t)d])) return rc3;
                return fs::mscg_dev_shift_dot(f.rows(d), sh.base, vp[(size_t)d], vq[(size_t)d], cg_sums(W, d, sums.send(d)), scalars_of(d),
                                              D->stream[d]);
              })) return rc2;
          if (int rc2 = combine(fs::kMscgS1)) return rc2;                       // alpha, the a_i
          if (int rc2 = each_rank(D, false, [&](int d) {
                return fs::mscg_dev_update(f.rows(d), W.r[(size_t)d], vp[(size_t)d], vq[(size_t)d], S.X[(size_t)d], ld, S.P[(size_t)d], ld,
                                           cg_sums(W, d, sums.send(d)), scalars_of(d), D->stream[d]);
              })) return rc2;
          if (int rc2 = combine(fs::kMscgS2)) return rc2;                       // converged?  beta, freezes
          if (int rc2 = each_rank(D, false, [&](int d) {
                return fs::mscg_dev_direction(f.rows(d), vp[(size_t)d], W.r[(size_t)d], S.P[(size_t)d], ld, W.st[(size_t)d], S.sc[(size_t)d],
                                              D->stream[d]);
              })) return rc2;
          return run_gather(D, exchange_of(M, true, 1), W.p, M->x, false);     // the new p on every rank
        })) return rc;
  }
  // every rank froze every shift at the same iteration in the same way: the per-shift array
  Agreement froze{{Outcome{S.sc, 0, (size_t)m * (fs::kMscgStateDoubles / FS_MSCG_MAX_SHIFTS)}}, [&](const double *mine, const double *first) {
    return fs::mscg_same_outcome(mine, first, m);
  }, "fs_dist_mscg: the devices froze the shifts differently (a device or an exchange returned different bits)", {}};
  if (int rc = f.finish(X, S.X, 1, &froze, m, (size_t)ld, (size_t)ldx)) return rc;
  fs::mscg_note_state(f.st0, froze.first.data(), m, info);
  return FS_OK;
}

// fs_mscgn across the ranks; the schemes are fs_dist_mscg's (option "dist_cg_scheme"):
//   0 "replicate"  every rank holds whole panels R, P, Q, the m X_i and the P_i and launches fs_mscgn's own steps on them
//                  (mscgn_dev_*): T = A P and Q = A' T are the sharded k-column products, no exchange for the sums.
//   1 "gather"     rank r keeps its rows of A' of R, Q, every X_i and every P_i; P and T = A P stay whole, the rank's slice of P is
//                  the k-column exchange's own send buffer.  The X_i and P_i never leave their rank: only P enters a product.
//                  Q_r = A'_r T is the rank's own shard product; q.p and r.r are the slice tree of fs_dist_cg per column
//                  (SliceSums), the scalar steps run on every rank over the gathered values; the new P is gathered.  The first P
//                  is B, which every rank holds whole after staging.
// The caller's X is written once, at the end, after every rank's {done, iterations}, mask of live columns and per-pair
// {live, converged, count} agreed.
int fs_dist_mscgn(fs_dist_matrix_t M, double *X, int64_t ldx, const double *B, int k, int m, const double *lambda, double tol, int max_iter,
                  fs_pcg_info *info)
{
  if (!M || !X || !B || !lambda) { fs::set_error("fs_dist_mscgn: NULL argument"); return FS_ERR_ARG; }
  if (k < 1 || k > FS_PCGN_MAX_RHS) { fs::set_error("fs_dist_mscgn: k outside 1..FS_PCGN_MAX_RHS"); return FS_ERR_ARG; }
  if (ldx < (int64_t)M->ncol * k) { fs::set_error("fs_dist_mscgn: ldx < ncol * k"); return FS_ERR_ARG; }
  if (int rc = fs::mscg_args_ok("fs_dist_mscgn", 0, ldx, m, lambda, tol)) return rc;     // (ldx is settled above)
  DistSolve f{"fs_dist_mscgn", M};
  if (int rc = f.open("call fs_dist_matrix_build_transpose first")) return rc;
  fs_dist_t D = f.D;
  const int F = f.F, n = f.n;
  const bool gather = fs::options().dist_cg_scheme == 1 && n > 1;
  const fs::MscgShifts sh = fs::mscg_shifts(m, lambda);
  const int cap = max_iter > 0 ? max_iter : F;               // cg.h:55
  f.slices(gather);
  if (k > 1)
    if (int rc = ensure_k(M, k)) return rc;
  if (int rc = ensure_pn_work(M, k, gather)) return rc;      // (ld: every X_i and P_i 16-byte aligned)
  if (int rc = ensure_ladder_work(M, M->mn, m, sh.nslots, ((long long)f.longest() * k + 1) & ~1LL, kMnScalarDoubles)) return rc;
  PnWork &W = M->pn;
  LadderWork &S = M->mn;
  const long long ld = S.ld;
  f.st = &W.st;
  const ProductVectors v = product_vectors(M, k);              // (Q as a whole panel: scheme 0 only)
  // the slice of P: the local output buffer of the A' side, which no product of scheme 1 writes -- the gather's own source
  const Exchange gp = exchange_of(M, true, k);
  const std::vector<double *> &dp = gather ? gp.local : v.p, &dq = gather ? W.q : v.q;
  auto scalars_of = [&](int d) {
    double *red = S.sc[(size_t)d], *cst = red + fs::kPcgnSendDoubles, *ms = cst + kMnCstDoubles;
    return fs::MscgnScalars{red, cst, ms, ms + fs::kMscgnStateDoubles, m, tol, &sh};
  };
  // PnWork's send slots and gathered values with fs_mscgn's scalar step behind the exchange, every rank over the same values.
  // Where rank d's launchers leave their sums: on slices in the send slot, on whole panels where the scalar steps read them
  SliceSums sums{M, W.send, W.all, fs::kPcgnSendDoubles};
  auto sums_of = [&](int d, bool slot) { return pn_sums(W, d, slot ? sums.send(d) : S.sc[(size_t)d]); };
  auto combine = [&](fs::MscgStep step) {
    return sums.combine((size_t)(step == fs::kMscgStart ? 2 : 1) * (size_t)k, [&](int d, const double *all) {
      return fs::mscgn_dev_rank_step(step, all, n, k, sums_of(d, true), scalars_of(d), D->stream[d]);
    });
  };
  if (int rc = f.stage(gather ? v.p : W.b, B, (size_t)F * k)) return rc;    // slices: the whole B is the first P, where the product reads it
  if (int rc = each_rank(D, false, [&](int d) -> int {
        if (int rc2 = fs::pcgn_dev_clear(W.cs[(size_t)d], D->stream[d])) return rc2;
        FS_HIP(hipMemsetAsync(S.sc[(size_t)d], 0, sizeof(double) * kMnScalarDoubles, D->stream[d]));   // unwritten slots read as 0 in the debug getter
        return FS_OK;
      })) return rc;
  if (gather)
    if (int rc = f.take_slices(W.b, v.p, k)) return rc;
  if (int rc = each_rank(D, false, [&](int d) {
        return fs::mscgn_dev_init(f.rows(d), k, W.b[(size_t)d], S.X[(size_t)d], ld, W.r[(size_t)d], dp[(size_t)d], dq[(size_t)d], S.P[(size_t)d], ld,
                                  sums_of(d, gather), scalars_of(d), D->stream[d]);
      })) return rc;
  if (gather)
    if (int rc = combine(fs::kMscgStart)) return rc;                         // b.b, r.r per column: stop, every pair's scalars, live?
  if (!gather) {
    if (int rc = f.iterate(cap, true, [&] { return dist_pair(M, k, v.p, v.t, v.q); }, [&](int d) {     // T = A P, Q = A' T
          return fs::mscgn_dev_steps(F, k, S.X[(size_t)d], ld, W.r[(size_t)d], v.p[(size_t)d], v.q[(size_t)d], S.P[(size_t)d], ld, sums_of(d, false),
                                     scalars_of(d), D->stream[d]);
        })) return rc;
  } else {
    if (int rc = f.iterate(cap, true, [&]() -> int {
          if (int rc2 = dist_product(M, false, k, v.p, v.t)) return rc2;     // T = A P
          if (int rc2 = each_rank(D, false, [&](int d) -> int {              // Q_r = A'_r T: the rank's own shard product
                if (int rc3 = f.shard_product(d, k, dq[(size_t)d], v.t[(size_t)d])) return rc3;
                return fs::mscgn_dev_shift_dot(f.rows(d), k, dq[(size_t)d], dp[(size_t)d], sums_of(d, true), scalars_of(d), D->stream[d]);
              })) return rc2;
          if (int rc2 = combine(fs::kMscgS1)) return rc2;                    // alpha_j, the a_ij
          if (int rc2 = each_rank(D, false, [&](int d) {
                return fs::mscgn_dev_update(f.rows(d), k, S.X[(size_t)d], ld, W.r[(size_t)d], dp[(size_t)d], dq[(size_t)d], S.P[(size_t)d], ld,
                                            sums_of(d, true), scalars_of(d), D->stream[d]);
              })) return rc2;
          if (int rc2 = combine(fs::kMscgS2)) return rc2;                    // converged?  beta_j, freezes
          if (int rc2 = each_rank(D, false, [&](int d) {
                return fs::mscgn_dev_direction(f.rows(d), k, dp[(size_t)d], W.r[(size_t)d], S.P[(size_t)d], ld, sums_of(d, true), scalars_of(d),
                                               D->stream[d]);
              })) return rc2;
          return run_gather(D, gp, dp, v.p, false);                          // the new P on every rank
        })) return rc;
  }
  // every rank froze every column and every pair at the same iteration in the same way: every column's st[] and ms[], then the
  // rank's st[] for the live mask
  const size_t ncst = (size_t)k * fs::kCgStateDoubles, nms = (size_t)k * fs::kMscgStateDoubles;
  Agreement froze{{Outcome{S.sc, (size_t)fs::kPcgnSendDoubles, ncst}, Outcome{S.sc, fs::kPcgnSendDoubles + kMnCstDoubles, nms},
                   Outcome{W.st, 0, (size_t)fs::kCgStateDoubles}}, [&](const double *mine, const double *first) {
    bool same = mine[ncst + nms + fs::kCgStateLiveMask] == first[ncst + nms + fs::kCgStateLiveMask];
    for (int j = 0; j < k; ++j)
      same = same && mine[(size_t)j * fs::kCgStateDoubles + fs::kCgStateDone] == first[(size_t)j * fs::kCgStateDoubles + fs::kCgStateDone] &&
             fs::mscg_same_outcome(mine + ncst + (size_t)j * fs::kMscgStateDoubles, first + ncst + (size_t)j * fs::kMscgStateDoubles, m);
    return same;
  }, "fs_dist_mscgn: the devices froze the pairs differently (a device or an exchange returned different bits)", {}};
  if (int rc = f.finish(X, S.X, k, &froze, m, (size_t)ld, (size_t)ldx)) return rc;
  fs::mscgn_note_state(froze.first.data(), froze.first.data() + ncst, k, m, info);
  return FS_OK;
}

// Y[nrow, k] = A X[ncol, k], row-major host matrices (csr_A_mul_Bn / bcsr_A_mul_Bn / bsbm_A_mul_Bn across the GPUs, csr.h:441,
// 257; sparse.h:318): every device multiplies its shard (the k-column kernels of fs_spmm, prepared on first use of a k) and the
// Y shards are all-gathered -- inside the product where the plan finishes rows part by part, else behind it (dist_product).
// fs_dist_spmm_t: Z[ncol, k] = A' U[nrow, k].
int fs_dist_spmm(fs_dist_matrix_t M, double *Y, const double *X, int k)
{
  if (!M || !Y || !X || k < 1) { fs::set_error("fs_dist_spmm: bad argument"); return FS_ERR_ARG; }
  if (k == 1) return fs_dist_spmv(M, Y, X);
  return dist_apply(M, false, Y, X, k);
}

int fs_dist_spmm_t(fs_dist_matrix_t M, double *Z, const double *U, int k)
{
  if (!M || !Z || !U || k < 1) { fs::set_error("fs_dist_spmm_t: bad argument"); return FS_ERR_ARG; }
  if (!M->t.built) { fs::set_error("fs_dist_spmm_t: build the transpose first"); return FS_ERR_NO_TRANSPOSE; }
  if (k == 1) return fs_dist_spmv_t(M, Z, U);
  return dist_apply(M, true, Z, U, k);
}

// (A'A + lambda I) X = B for two right-hand sides, row-major ncol x 2: bsbm_cg2 (cg.h:85-187) across the GPUs.  Every device
// keeps whole X, R, P, Q and runs the same block-CG steps on them (identical inputs, identical kernels: the 2x2 algebra needs no
// exchange); per iteration TMP = A P and Q = A' TMP as two-column products with their all-gathers.
int fs_dist_cg2(fs_dist_matrix_t M, double *X_host, const double *B_host, double lambda, double tol, int *out_iter)
{
  if (!M || !X_host || !B_host) { fs::set_error("fs_dist_cg2: NULL argument"); return FS_ERR_ARG; }
  DistSolve f{"fs_dist_cg2", M};
  if (int rc = f.open("build the transpose first")) return rc;
  fs_dist_t D = f.D;
  const int F = f.F;
  if (int rc = ensure_k(M, 2)) return rc;
  KWork &W = M->kw;
  f.st = &W.st;
  if (int rc = f.stage(W.b, B_host, (size_t)F * 2)) return rc;
  std::vector<double> norms(2 * (size_t)f.n, 0.0);           // cg2_dev_init is synchronous: the norms of B's columns, per rank
  if (int rc = each_rank(D, false, [&](int d) -> int {
        if (int rc2 = fs::cg2_dev_init(F, W.b[(size_t)d], W.sol[(size_t)d], W.r[(size_t)d], W.x[(size_t)d], W.part[(size_t)d], W.red[(size_t)d],
                                       W.st[(size_t)d], tol, &norms[2 * (size_t)d], D->stream[d])) return rc2;
        if (norms[2 * (size_t)d] != norms[0] || norms[2 * (size_t)d + 1] != norms[1]) {
          fs::set_error("fs_dist_cg2: the devices disagree about the norms of the right-hand sides");
          return FS_ERR_HIP;
        }
        return FS_OK;
      })) return rc;
  if (int rc = f.iterate(F, false, [&] { return dist_pair(M, 2, W.x, W.y, W.z); }, [&](int d) {     // TMP = A P, Q = A' TMP
        return fs::cg2_dev_steps(F, lambda, W.sol[(size_t)d], W.r[(size_t)d], W.x[(size_t)d], W.z[(size_t)d], W.part[(size_t)d],
                                 W.red[(size_t)d], W.st[(size_t)d], D->stream[d]);
      })) return rc;
  if (f.seen != kRanksDisagree)                              // X back in B's scale
    if (int rc = each_rank(D, false, [&](int d) { return fs::cg2_dev_finish(F, &norms[2 * (size_t)d], W.sol[(size_t)d], D->stream[d]); })) return rc;
  if (int rc = f.finish(X_host, W.sol, 2)) return rc;
  if (out_iter) *out_iter = f.iterations;
  return FS_OK;
}

double *fs_dist_x(fs_dist_matrix_t M, int rank) { return (M && rank >= 0 && rank < M->D->n) ? M->x[(size_t)rank] : nullptr; }
double *fs_dist_y(fs_dist_matrix_t M, int rank) { return (M && rank >= 0 && rank < M->D->n) ? M->y[(size_t)rank] : nullptr; }
double *fs_dist_z(fs_dist_matrix_t M, int rank) { return (M && rank >= 0 && rank < M->D->n) ? M->z[(size_t)rank] : nullptr; }

// diagnostics, not in include/fastsparse_hip.h: rank's resident copy of the k-column X (0), Y (1) or Z (2) of the handle's current
// k -- what fs_dist_x / _y / _z are to the single-vector products -- or NULL before the first k-column product
double *fs_debug_dist_k_vector(fs_dist_matrix_t M, int rank, int which)
{
  if (!M || !M->kw.mem.ready || rank < 0 || rank >= M->D->n || which < 0 || which > 2) return nullptr;
  return (which == 0 ? M->kw.x : which == 1 ? M->kw.y : M->kw.z)[(size_t)rank];
}

}  // extern "C"
