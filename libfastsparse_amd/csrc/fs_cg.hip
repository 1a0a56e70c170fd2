// fs_cg.hip -- the consumers of the A_mul_B path, device resident:
// conjugate gradients on (A'A + lambda I) with one right-hand side (bsbm_cg, cg.h:25-82) and with two
// row-major right-hand sides (bsbm_cg2, cg.h:85-187).  Every vector lives in HBM for the whole solve; per
// iteration two products (fs_spmv / fs_spmm on A and A') and three fused vector kernels run.  The scalars of the
// iteration (alpha, beta, r.r; for two right-hand sides the 2x2 algebra of solve2sym, linalg.h:77-88) are computed
// ON THE DEVICE by the one-workgroup kernel that finishes each reduction, with the reference's formulas, and stay
// there: nothing in an iteration waits for the host.  The host only has to learn WHEN to stop enqueuing: the
// "done" flag of iteration i is copied to pinned memory behind it and looked at while iteration i + 1 runs; the
// vector kernels of iterations enqueued past the end see the flag and do nothing (their products are wasted
// work: at most two iterations' worth).  Fetching every reduction to the host instead costs two stream
// synchronisations per iteration, 0.1-0.2 ms of idle GPU in a 1.5 ms iteration.
//
// Reductions are two-stage with a fixed shape (1024 workgroup partials, then one workgroup), so results are
// reproducible run to run; they are NOT the CPU's single left-to-right sums, so iterates agree with the
// reference to rounding, not bit for bit.
#include <math.h>

#include <vector>

#include "fs_common.h"
#include "fs_pcgn_plan.h"

namespace fs {

constexpr int kRedBlocks = 1024;
constexpr int kRedThreads = 256;

// sum of NV values per thread over the workgroup -> part[blockIdx * NV + j]
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double *__restrict__ part)
{
  __shared__ double sm[NV][kRedThreads / 64];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    double s = v[j];
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
    if ((threadIdx.x & 63) == 0) sm[j][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double s = 0.0;
    for (int w = 0; w < kRedThreads / 64; ++w) s += sm[threadIdx.x][w];
    part[blockIdx.x * NV + threadIdx.x] = s;
  }
}

// the one workgroup that finishes a reduction: the nblocks partials of stage 1 -> red[0..NV), which every thread may read on
// return (SYNC; a kernel that ends here needs no barrier)
template <int NV, bool SYNC = true>
__device__ __forceinline__ void finish_sum(const double *__restrict__ part, int nblocks, double *__restrict__ red)
{
  double v[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    v[j] = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kRedThreads) v[j] += part[b * NV + j];
  }
  block_sum<NV>(v, red);  // gridDim == 1: red[0..NV)
  if (SYNC) __syncthreads();
}

template <int NV>
__global__ __launch_bounds__(kRedThreads) void final_sum_kernel(const double *__restrict__ part, int nblocks,
                                                               double *__restrict__ out)
{
  finish_sum<NV, false>(part, nblocks, out);
}

// ---- one right-hand side --------------------------------------------------------------------------------
// x = 0, r = p = b, partial b.b                                   (cg.h:46-51)
__global__ __launch_bounds__(kRedThreads) void cg_init_kernel(int n, const double *__restrict__ b, double *__restrict__ x,
                                                             double *__restrict__ r, double *__restrict__ p,
                                                             double *__restrict__ part)
{
  double v[1] = {0.0};
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    const double bi = b[i];
    x[i] = 0.0; r[i] = bi; p[i] = bi;
    v[0] += bi * bi;
  }
  block_sum<1>(v, part);
}

// ---- two right-hand sides, row-major -------------------------------------------------------------------
// partial {a'a, b'b, a'b} of X with Y                             (pnormsq2 / pouter2 / pdot2sym, linalg.h:24-73)
__global__ __launch_bounds__(kRedThreads) void cg2_dot_kernel(int n, const double *__restrict__ X,
                                                             const double *__restrict__ Y, double *__restrict__ part)
{
  double v[3] = {0.0, 0.0, 0.0};
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    const double xa = X[2 * i], xb = X[2 * i + 1], ya = Y[2 * i], yb = Y[2 * i + 1];
    v[0] += xa * ya; v[1] += xb * yb; v[2] += xa * yb;
  }
  block_sum<3>(v, part);
}

// X = 0, R = P = B * inorms, partial R'R                          (cg.h:113-125)
__global__ __launch_bounds__(kRedThreads) void cg2_init_kernel(int n, double in0, double in1, const double *__restrict__ B,
                                                              double *__restrict__ X, double *__restrict__ R,
                                                              double *__restrict__ P, double *__restrict__ part)
{
  double v[3] = {0.0, 0.0, 0.0};
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    const double a = B[2 * i] * in0, c = B[2 * i + 1] * in1;
    X[2 * i] = 0.0; X[2 * i + 1] = 0.0;
    R[2 * i] = a; R[2 * i + 1] = c; P[2 * i] = a; P[2 * i + 1] = c;
    v[0] += a * a; v[1] += c * c; v[2] += a * c;
  }
  block_sum<3>(v, part);
}

// y += a x
__global__ __launch_bounds__(kRedThreads) void axpy_kernel(int n, double a, const double *__restrict__ x, double *__restrict__ y)
{
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) y[i] += a * x[i];
}

__global__ __launch_bounds__(kRedThreads) void cg2_scale_kernel(int n, double n0, double n1, double *__restrict__ X)
{
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    X[2 * i] *= n0;
    X[2 * i + 1] *= n1;
  }
}

// ---- the steps of an iteration, their scalars in device memory ---------------------------------------------
// state of one solve, doubles.  One right-hand side: rsq_old, alpha, beta, stop; two: RtR[3], Alpha[4], Psi[4], tolsq
// fs_pcg: kStRsq holds r.z (rsq_old's role), kStRr the recurrence's last r.r, kStBb b.b
enum { kStDone = kCgStateDone, kStIter = kCgStateIter, kStRsq = 2, kStAlpha = 3, kStBeta = 4, kStStop = 5, kStRr = 6, kStBb = 7,
       kSt2RtR = 2, kSt2Alpha = 5, kSt2Psi = 9, kSt2Tolsq = 13, kStDoubles = kCgStateDoubles };

__device__ __forceinline__ void solve2sym_dev(double *X, const double *A, const double *RHS)  // linalg.h:77-88
{
  const double dinv = 1.0 / (A[0] * A[1] - A[2] * A[2]);
  const double i0 = dinv * A[1], i1 = dinv * A[0], i2 = -dinv * A[2];
  X[0] = i0 * RHS[0] + i2 * RHS[1];
  X[1] = i2 * RHS[0] + i1 * RHS[1];
  X[2] = i0 * RHS[2] + i2 * RHS[3];
  X[3] = i2 * RHS[2] + i1 * RHS[3];
}

// the one workgroup that finishes a reduction, then does the iteration's scalar step STEP (CgStep, fs_common.h; cg.h:59-76,
// 143-172).  tol in `arg` for the two start steps.  fs_pcg keeps r.z in kStRsq; its steps run with NV = 1 without a
// preconditioner, where z is r and r.z is r.r
template <int NV, CgStep STEP>
__global__ __launch_bounds__(kRedThreads) void final_step_kernel(const double *__restrict__ part, int nblocks,
                                                                double *__restrict__ red, double *__restrict__ st, double arg)
{
  if (STEP != kStepCgStart && STEP != kStepPcgStart && st[kStDone] != 0.0) return;
  finish_sum<NV>(part, nblocks, red);
  if (threadIdx.x != 0) return;
  if (STEP == kStepCgStart) {
    st[kStRsq] = red[0]; st[kStStop] = arg * sqrt(red[0]); st[kStDone] = 0.0; st[kStIter] = 0.0;
  } else if (STEP == kStepCgAlpha) {
    st[kStAlpha] = st[kStRsq] / red[0];
  } else if (STEP == kStepCgBeta) {
    const double rsq_new = red[0];
    if (sqrt(rsq_new) <= st[kStStop]) st[kStDone] = 1.0;
    else { st[kStBeta] = rsq_new / st[kStRsq]; st[kStRsq] = rsq_new; st[kStIter] += 1.0; }
  } else if (STEP == kStepCg2Alpha) {
    const double rhs[4] = {st[kSt2RtR], st[kSt2RtR + 2], st[kSt2RtR + 2], st[kSt2RtR + 1]};
    double a[4];
    solve2sym_dev(a, red, rhs);
    st[kSt2Alpha] = a[0]; st[kSt2Alpha + 1] = a[1]; st[kSt2Alpha + 2] = a[2]; st[kSt2Alpha + 3] = a[3];
  } else if (STEP == kStepCg2Psi) {
    const double n0 = red[0], n1 = red[1], n2 = red[2], tolsq = st[kSt2Tolsq];
    if (n0 <= tolsq && n1 <= tolsq) st[kStDone] = 1.0;
    else {
      const double old[3] = {st[kSt2RtR], st[kSt2RtR + 1], st[kSt2RtR + 2]};
      const double rhs[4] = {n0, n2, n2, n1};
      double ps[4];
      solve2sym_dev(ps, old, rhs);
      st[kSt2Psi] = ps[0]; st[kSt2Psi + 1] = ps[1]; st[kSt2Psi + 2] = ps[2]; st[kSt2Psi + 3] = ps[3];
      st[kSt2RtR] = n0; st[kSt2RtR + 1] = n1; st[kSt2RtR + 2] = n2;
      st[kStIter] += 1.0;
    }
  } else if (STEP == kStepPcgStart) {
    const double stop = arg * sqrt(red[0]);
    st[kStBb] = red[0]; st[kStRr] = red[1]; st[kStStop] = stop; st[kStIter] = 0.0;
    st[kStDone] = sqrt(red[1]) <= stop ? 1.0 : 0.0;
  } else if (STEP == kStepPcgRz) {
    st[kStRsq] = red[0];
  } else if (STEP == kStepPcgBeta) {
    const double rr = red[0], rz_new = red[NV - 1];
    st[kStRr] = rr;
    if (sqrt(rr) <= st[kStStop]) st[kStDone] = 1.0;
    else { st[kStBeta] = rz_new / st[kStRsq]; st[kStRsq] = rz_new; st[kStIter] += 1.0; }
  }
}

// q += lambda p, partial q.p                                      (cg.h:17-21, :59)
__global__ __launch_bounds__(kRedThreads) void cg_shift_dot_dev_kernel(int n, double lambda, double *__restrict__ q,
                                                                      const double *__restrict__ p, double *__restrict__ part,
                                                                      const double *__restrict__ st)
{
  if (st[kStDone] != 0.0) return;
  double v[1] = {0.0};
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    const double pi = p[i];
    const double qi = q[i] + lambda * pi;
    q[i] = qi;
    v[0] += qi * pi;
  }
  block_sum<1>(v, part);
}

// x += alpha p, r -= alpha q, partial r.r                         (cg.h:61-67)
__global__ __launch_bounds__(kRedThreads) void cg_update_dev_kernel(int n, double *__restrict__ x, double *__restrict__ r,
                                                                   const double *__restrict__ p, const double *__restrict__ q,
                                                                   double *__restrict__ part, const double *__restrict__ st)
{
  if (st[kStDone] != 0.0) return;
  const double alpha = st[kStAlpha];
  double v[1] = {0.0};
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    x[i] += alpha * p[i];
    const double ri = r[i] - alpha * q[i];
    r[i] = ri;
    v[0] += ri * ri;
  }
  block_sum<1>(v, part);
}

// p = r + beta p                                                  (cg.h:71-75)
__global__ __launch_bounds__(kRedThreads) void cg_direction_dev_kernel(int n, double *__restrict__ p, const double *__restrict__ r,
                                                                      const double *__restrict__ st)
{
  if (st[kStDone] != 0.0) return;
  const double beta = st[kStBeta];
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) p[i] = r[i] + beta * p[i];
}

// Q += lambda P, partial P'Q (symmetric form)                      (cg.h:136-142)
__global__ __launch_bounds__(kRedThreads) void cg2_shift_dot_dev_kernel(int n, double lambda, double *__restrict__ Q,
                                                                       const double *__restrict__ P, double *__restrict__ part,
                                                                       const double *__restrict__ st)
{
  if (st[kStDone] != 0.0) return;
  double v[3] = {0.0, 0.0, 0.0};
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    const double pa = P[2 * i], pb = P[2 * i + 1];
    const double qa = Q[2 * i] + lambda * pa, qb = Q[2 * i + 1] + lambda * pb;
    Q[2 * i] = qa; Q[2 * i + 1] = qb;
    v[0] += pa * qa; v[1] += pb * qb; v[2] += pa * qb;
  }
  block_sum<3>(v, part);
}

// X += Alpha' P, R -= Alpha' Q, partial R'R                        (cg.h:148-157)
__global__ __launch_bounds__(kRedThreads) void cg2_update_dev_kernel(int n, double *__restrict__ X, double *__restrict__ R,
                                                                    const double *__restrict__ P, const double *__restrict__ Q,
                                                                    double *__restrict__ part, const double *__restrict__ st)
{
  if (st[kStDone] != 0.0) return;
  const double a0 = st[kSt2Alpha], a1 = st[kSt2Alpha + 1], a2 = st[kSt2Alpha + 2], a3 = st[kSt2Alpha + 3];
  double v[3] = {0.0, 0.0, 0.0};
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    const double pa = P[2 * i], pb = P[2 * i + 1], qa = Q[2 * i], qb = Q[2 * i + 1];
    X[2 * i] += a0 * pa + a1 * pb;
    X[2 * i + 1] += a2 * pa + a3 * pb;
    const double ra = R[2 * i] - (a0 * qa + a1 * qb), rb = R[2 * i + 1] - (a2 * qa + a3 * qb);
    R[2 * i] = ra; R[2 * i + 1] = rb;
    v[0] += ra * ra; v[1] += rb * rb; v[2] += ra * rb;
  }
  block_sum<3>(v, part);
}

// P = R + Psi' P                                                   (cg.h:165-171)
__global__ __launch_bounds__(kRedThreads) void cg2_direction_dev_kernel(int n, double *__restrict__ P, const double *__restrict__ R,
                                                                       const double *__restrict__ st)
{
  if (st[kStDone] != 0.0) return;
  const double s0 = st[kSt2Psi], s1 = st[kSt2Psi + 1], s2 = st[kSt2Psi + 2], s3 = st[kSt2Psi + 3];
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    const double pa = P[2 * i], pb = P[2 * i + 1];
    P[2 * i] = R[2 * i] + s0 * pa + s1 * pb;
    P[2 * i + 1] = R[2 * i + 1] + s2 * pa + s3 * pb;
  }
}

// ---- fs_pcg: Jacobi-preconditioned CG with a warm start (one right-hand side) ----------------------------------------
// d[row] = lambda + sum of v^2 over the row (v = 1 for a pattern-only matrix): one wave per row, the grid strides over the rows.
// Lane l adds v * v of entries l, l + 64, ... to +0.0 in that order, the wave folds like block_sum, lambda goes in last.
__global__ __launch_bounds__(kRedThreads) void gram_diag_kernel(int nrow, const int *__restrict__ row_ptr,
                                                               const double *__restrict__ vals, double lambda,
                                                               double *__restrict__ d)
{
  const int lane = threadIdx.x & 63;
  const int nwaves = gridDim.x * (kRedThreads / 64);
  for (int row = blockIdx.x * (kRedThreads / 64) + (threadIdx.x >> 6); row < nrow; row += nwaves) {   // (wave-uniform)
    const int lo = row_ptr[row], hi = row_ptr[row + 1];
    double s = 0.0;
    for (int e = lo + lane; e < hi; e += 64) {
      const double v = vals ? vals[e] : 1.0;
      s += v * v;
    }
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) d[row] = s + lambda;
  }
}

// dinv = 1 / d, 1 where d is 0 (an empty column with lambda = 0: r stays, as without a preconditioner); in place or not
__global__ __launch_bounds__(kRedThreads) void pcg_dinv_kernel(int n, const double *d, double *dinv)
{
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    const double di = d[i];
    dinv[i] = di == 0.0 ? 1.0 : 1.0 / di;
  }
}

// cold: x = 0, r = b.  warm (q = A'(A x) on entry): q += lambda x, r = b - q.  Partials {b.b, r.r}
template <bool WARM>
__global__ __launch_bounds__(kRedThreads) void pcg_init_kernel(int n, double lambda, const double *__restrict__ b,
                                                              double *__restrict__ x, double *__restrict__ r,
                                                              double *__restrict__ q, double *__restrict__ part)
{
  double v[2] = {0.0, 0.0};
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    const double bi = b[i];
    double ri = bi;
    if (WARM) {
      const double qi = q[i] + lambda * x[i];
      q[i] = qi;
      ri = bi - qi;
    } else {
      x[i] = 0.0;
    }
    r[i] = ri;
    v[0] += bi * bi; v[1] += ri * ri;
  }
  block_sum<2>(v, part);
}

// p = z = r dinv (PRE) or r, partial r.z
template <bool PRE>
__global__ __launch_bounds__(kRedThreads) void pcg_start_kernel(int n, const double *__restrict__ r, const double *__restrict__ dinv,
                                                               double *__restrict__ p, double *__restrict__ part,
                                                               const double *__restrict__ st)
{
  if (st[kStDone] != 0.0) return;
  double v[1] = {0.0};
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    const double ri = r[i];
    const double zi = PRE ? ri * dinv[i] : ri;
    p[i] = zi;
    v[0] += ri * zi;
  }
  block_sum<1>(v, part);
}

// x += alpha p, r -= alpha q, z = r dinv, partials {r.r, r.z} in one pass (without a preconditioner: cg_update_dev_kernel)
__global__ __launch_bounds__(kRedThreads) void pcg_update_kernel(int n, double *__restrict__ x, double *__restrict__ r,
                                                                const double *__restrict__ p, const double *__restrict__ q,
                                                                const double *__restrict__ dinv, double *__restrict__ part,
                                                                const double *__restrict__ st)
{
  if (st[kStDone] != 0.0) return;
  const double alpha = st[kStAlpha];
  double v[2] = {0.0, 0.0};
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    x[i] += alpha * p[i];
    const double ri = r[i] - alpha * q[i];
    r[i] = ri;
    const double zi = ri * dinv[i];
    v[0] += ri * ri; v[1] += ri * zi;
  }
  block_sum<2>(v, part);
}

// p = z + beta p with z = r dinv formed on the fly: no z vector is stored (without a preconditioner: cg_direction_dev_kernel)
__global__ __launch_bounds__(kRedThreads) void pcg_direction_kernel(int n, double *__restrict__ p, const double *__restrict__ r,
                                                                   const double *__restrict__ dinv, const double *__restrict__ st)
{
  if (st[kStDone] != 0.0) return;
  const double beta = st[kStBeta];
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    const double zi = r[i] * dinv[i];
    p[i] = zi + beta * p[i];
  }
}

// ---- fs_mscg: multi-shift CG, (A'A + lambda_i I) x_i = b for up to kMscgMaxShifts lambdas from ONE Krylov sequence ---------
// The base system (the smallest lambda) runs fs_cg's iteration on fs_cg's kernels and bits; every other shift sigma_i = lambda_i -
// base follows by scalar recurrences (include/fastsparse_hip.h spells the arithmetic out).  st[] keeps the base scalars, ms[] the
// per-shift ones, kMsStride doubles each.  ms[k * kMsStride + kMsList], k < st[kStNBase] + st[kStNLive], is the compacted list of
// live shifts: those with sigma = 0 first (their direction IS p: no vector of their own), then the others (direction P + pslot ldp).
constexpr int kMscgMaxShifts = FS_MSCG_MAX_SHIFTS;
enum { kStAprev = 8, kStBprev = 9, kStNLive = 10, kStNBase = 11 };
enum { kMsSigma = 0, kMsZ = 1, kMsZp = 2, kMsZn = 3, kMsRatio = 4, kMsA = 5, kMsB = 6, kMsRn = 7, kMsLive = 8, kMsConverged = 9,
       kMsCount = 10, kMsList = 11, kMsPslot = 12, kMsStride = 16 };
constexpr int kMscgGroup = 4;              // shifts whose loads one thread keeps in flight together
static_assert(kMscgStateDoubles == kMscgMaxShifts * kMsStride, "fs_common.h sizes the callers' ms[]");

// x_i = 0 for the m shifts, r = p = b, P = b for the nslots shifts with sigma != 0, partial b.b
__global__ __launch_bounds__(kRedThreads) void mscg_init_kernel(int n, const double *__restrict__ b, double *__restrict__ r,
                                                               double *__restrict__ p, double *X, long long ldx, int m, double *P,
                                                               long long ldp, int nslots, double *__restrict__ part)
{
  double v[1] = {0.0};
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    const double bi = b[i];
    r[i] = bi; p[i] = bi;
    for (int j = 0; j < m; ++j) X[j * ldx + i] = 0.0;
    for (int j = 0; j < nslots; ++j) P[j * ldp + i] = bi;
    v[0] += bi * bi;
  }
  block_sum<1>(v, part);
}

// the compacted list of live shifts, by one thread: sigma = 0 first, then the others, each in the caller's order
__device__ __forceinline__ void mscg_list(int m, double *__restrict__ st, double *__restrict__ ms)
{
  int nb = 0, nl = 0;
  for (int i = 0; i < m; ++i)
    if (ms[i * kMsStride + kMsLive] != 0.0 && ms[i * kMsStride + kMsSigma] == 0.0) ms[(nb++) * kMsStride + kMsList] = (double)i;
  for (int i = 0; i < m; ++i)
    if (ms[i * kMsStride + kMsLive] != 0.0 && ms[i * kMsStride + kMsSigma] != 0.0) ms[(nb + nl++) * kMsStride + kMsList] = (double)i;
  st[kStNBase] = (double)nb; st[kStNLive] = (double)nl;
  if (nb + nl == 0) st[kStDone] = 1.0;     // nothing left to iterate for (besides convergence: every shift frozen by a NaN)
}

// The three scalar steps as the work of one thread per shift (`lane`) on one right-hand side's st[] and ms[]: fs_mscg's kernels run
// them with lane = threadIdx.x, fs_mscgn's run one per column side by side.  Every thread of the workgroup calls a step (it holds
// barriers); `active` false: this thread's right-hand side takes no part (fs_mscgn: a frozen column, a lane past the last column).

// start: stop, the scalars of the base system and of every shift
__device__ __forceinline__ void mscg_start_step(double bb, double tol, double *__restrict__ st, double *__restrict__ ms, int m,
                                                const MscgSigma &sg, int lane, bool active)
{
  const double stop = tol * sqrt(bb);
  const bool done = sqrt(bb) <= stop;
  if (active && lane < m) {
    double *e = ms + lane * kMsStride;
    e[kMsSigma] = sg.v[lane];
    e[kMsZ] = 1.0; e[kMsZp] = 1.0; e[kMsZn] = 1.0; e[kMsRatio] = 1.0; e[kMsA] = 0.0; e[kMsB] = 0.0;
    e[kMsRn] = sqrt(bb); e[kMsLive] = done ? 0.0 : 1.0; e[kMsConverged] = done ? 1.0 : 0.0; e[kMsCount] = 0.0;
    e[kMsList] = -1.0; e[kMsPslot] = -1.0;
  }
  __syncthreads();
  if (!active || lane != 0) return;
  st[kStBb] = bb; st[kStRr] = bb; st[kStRsq] = bb; st[kStStop] = stop; st[kStIter] = 0.0; st[kStDone] = done ? 1.0 : 0.0;
  st[kStAprev] = 1.0; st[kStBprev] = 0.0;
  int slots = 0;
  for (int i = 0; i < m; ++i)
    if (ms[i * kMsStride + kMsSigma] != 0.0) ms[i * kMsStride + kMsPslot] = (double)(slots++);
  if (done) { st[kStNBase] = 0.0; st[kStNLive] = 0.0; }
  else mscg_list(m, st, ms);
}

// S1: alpha = rsq / q.p (red[0]), then per live shift zn, ratio and the step a_i
__device__ __forceinline__ void mscg_s1_step(const double *__restrict__ red, double *__restrict__ st, double *__restrict__ ms, int m,
                                             int lane, bool active)
{
  const double alpha = st[kStRsq] / red[0];
  if (!active) return;
  if (lane == 0) st[kStAlpha] = alpha;
  if (lane >= m) return;
  double *e = ms + lane * kMsStride;
  if (e[kMsLive] == 0.0) return;
  const double aprev = st[kStAprev], bprev = st[kStBprev], sigma = e[kMsSigma], z = e[kMsZ], zp = e[kMsZp];
  double u = alpha * bprev; u = u * (zp - z);
  double w = sigma * alpha; w = 1.0 + w;
  double v = zp * aprev; v = v * w;
  const double den = u + v;
  double zn = z * zp; zn = zn * aprev; zn = zn / den;
  const double ratio = zn / z;
  e[kMsZn] = zn; e[kMsRatio] = ratio; e[kMsA] = alpha * ratio;
}

// S2: r.r is red[0]; the base system's convergence test and beta (fs_cg's kStepCgBeta, fs_pcg's r.r kept); per live shift its
// residual norm, freeze or b_i and the new z; then the list of the shifts that stay live
__device__ __forceinline__ void mscg_s2_step(const double *__restrict__ red, double *__restrict__ st, double *__restrict__ ms, int m,
                                             int lane, bool active)
{
  const double rr = red[0], rsq = st[kStRsq], stop = st[kStStop], alpha = st[kStAlpha], n = st[kStIter];
  const double s = sqrt(rr);
  const bool done = s <= stop;
  const double beta = rr / rsq;
  __syncthreads();                         // every thread has read st[] before lane 0 moves it on
  if (active && lane == 0) {
    st[kStRr] = rr;
    if (done) st[kStDone] = 1.0;
    else { st[kStBeta] = beta; st[kStRsq] = rr; st[kStIter] = n + 1.0; st[kStAprev] = alpha; st[kStBprev] = beta; }
  }
  if (active && lane < m) {
    double *e = ms + lane * kMsStride;
    if (e[kMsLive] != 0.0) {
      const double zn = e[kMsZn], ratio = e[kMsRatio];
      const double rn = fabs(zn) * s;
      e[kMsRn] = rn;
      if (!(rn > stop) || fabs(zn) < 0x1p-500 || done) {
        e[kMsLive] = 0.0; e[kMsConverged] = rn <= stop ? 1.0 : 0.0; e[kMsCount] = n;
      } else {
        double bi = ratio * ratio; bi = beta * bi;
        e[kMsB] = bi; e[kMsZp] = e[kMsZ]; e[kMsZ] = zn; e[kMsCount] = n + 1.0;
      }
    }
  }
  __syncthreads();
  if (active && lane == 0 && !done) mscg_list(m, st, ms);
}

// start: b.b, stop, the scalars of the base system and of every shift (one thread per shift)
__global__ __launch_bounds__(kRedThreads) void mscg_start_kernel(const double *__restrict__ part, int nblocks, double *__restrict__ red,
                                                                double *__restrict__ st, double *__restrict__ ms, double tol, int m,
                                                                MscgSigma sg)
{
  finish_sum<1>(part, nblocks, red);
  mscg_start_step(red[0], tol, st, ms, m, sg, (int)threadIdx.x, true);
}

// S1: finishes q.p, alpha = rsq / q.p, then per live shift (one thread each) zn, ratio and the step a_i
__global__ __launch_bounds__(kRedThreads) void mscg_s1_kernel(const double *__restrict__ part, int nblocks, double *__restrict__ red,
                                                             double *__restrict__ st, double *__restrict__ ms, int m)
{
  if (st[kStDone] != 0.0) return;
  finish_sum<1>(part, nblocks, red);
  mscg_s1_step(red, st, ms, m, (int)threadIdx.x, true);
}

// update: r = r - alpha q with the partials of r.r in cg_update_dev_kernel's shape, x_i = x_i + a_i P_i for every live shift, kMscgGroup
// shifts at a time (CNT of them in this group: their loads are in flight together); the first group rides in the pass over r and
// q (FIRST).  A shift with sigma = 0 reads p.  Frozen shifts are not in the list: they cost no traffic.
template <int CNT, bool FIRST>
__device__ __forceinline__ void mscg_update_group(int n, int k0, double alpha, double *__restrict__ r, const double *__restrict__ p,
                                                  const double *__restrict__ q, double *X, long long ldx, const double *P,
                                                  long long ldp, const double *__restrict__ ms, double &sum)
{
  double av[CNT + 1]; double *xp[CNT + 1]; const double *pp[CNT + 1];
#pragma unroll
  for (int u = 0; u < CNT; ++u) {
    const int sh = __builtin_amdgcn_readfirstlane((int)ms[(k0 + u) * kMsStride + kMsList]);
    const int slot = __builtin_amdgcn_readfirstlane((int)ms[sh * kMsStride + kMsPslot]);
    av[u] = ms[sh * kMsStride + kMsA];
    xp[u] = X + sh * ldx;
    pp[u] = slot < 0 ? p : P + slot * ldp;
  }
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    double pv[CNT + 1], xv[CNT + 1];
#pragma unroll
    for (int u = 0; u < CNT; ++u) { pv[u] = pp[u][i]; xv[u] = xp[u][i]; }
    if (FIRST) {
      const double ri = r[i] - alpha * q[i];
      r[i] = ri;
      sum += ri * ri;
    }
#pragma unroll
    for (int u = 0; u < CNT; ++u) xp[u][i] = xv[u] + av[u] * pv[u];
  }
}

template <bool FIRST, typename... T>
__device__ __forceinline__ void mscg_update_groups(int cnt, T &&...a)
{
  if (cnt >= 4)      mscg_update_group<4, FIRST>(a...);
  else if (cnt == 3) mscg_update_group<3, FIRST>(a...);
  else if (cnt == 2) mscg_update_group<2, FIRST>(a...);
  else if (cnt == 1) mscg_update_group<1, FIRST>(a...);
  else if (FIRST)    mscg_update_group<0, FIRST>(a...);
}

__global__ __launch_bounds__(kRedThreads) void mscg_update_kernel(int n, double *__restrict__ r, const double *__restrict__ p,
                                                                 const double *__restrict__ q, double *X, long long ldx,
                                                                 const double *P, long long ldp, double *__restrict__ part,
                                                                 const double *__restrict__ st, const double *__restrict__ ms)
{
  static_assert(kMscgGroup == 4, "mscg_update_groups dispatches on 0..4");
  if (st[kStDone] != 0.0) return;
  const double alpha = st[kStAlpha];
  const int nall = __builtin_amdgcn_readfirstlane((int)st[kStNBase] + (int)st[kStNLive]);
  double v[1] = {0.0};
  mscg_update_groups<true>(nall, n, 0, alpha, r, p, q, X, ldx, P, ldp, ms, v[0]);
  for (int k0 = kMscgGroup; k0 < nall; k0 += kMscgGroup) mscg_update_groups<false>(nall - k0, n, k0, alpha, r, p, q, X, ldx, P, ldp, ms, v[0]);
  block_sum<1>(v, part);
}

// S2: finishes r.r, then mscg_s2_step
__global__ __launch_bounds__(kRedThreads) void mscg_s2_kernel(const double *__restrict__ part, int nblocks, double *__restrict__ red,
                                                             double *__restrict__ st, double *__restrict__ ms, int m)
{
  if (st[kStDone] != 0.0) return;
  finish_sum<1>(part, nblocks, red);
  mscg_s2_step(red, st, ms, m, (int)threadIdx.x, true);
}

// direction: p = r + beta p, P_i = z_i r + b_i P_i for every live shift with sigma != 0 (z_i the new one), kMscgGroup shifts at a
// time; the first group rides in the pass over r and p (FIRST).  `at` is the group's place in the list.
template <int CNT, bool FIRST>
__device__ __forceinline__ void mscg_direction_group(int n, int at, double beta, double *__restrict__ p, const double *__restrict__ r,
                                                     double *P, long long ldp, const double *__restrict__ ms)
{
  double zv[CNT + 1], bv[CNT + 1]; double *pp[CNT + 1];
#pragma unroll
  for (int u = 0; u < CNT; ++u) {
    const int sh = __builtin_amdgcn_readfirstlane((int)ms[(at + u) * kMsStride + kMsList]);
    const int slot = __builtin_amdgcn_readfirstlane((int)ms[sh * kMsStride + kMsPslot]);
    zv[u] = ms[sh * kMsStride + kMsZ]; bv[u] = ms[sh * kMsStride + kMsB];
    pp[u] = P + slot * ldp;
  }
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    double pv[CNT + 1];
#pragma unroll
    for (int u = 0; u < CNT; ++u) pv[u] = pp[u][i];
    const double ri = r[i];
    if (FIRST) p[i] = ri + beta * p[i];
#pragma unroll
    for (int u = 0; u < CNT; ++u) { const double t1 = zv[u] * ri, t2 = bv[u] * pv[u]; pp[u][i] = t1 + t2; }
  }
}

template <bool FIRST, typename... T>
__device__ __forceinline__ void mscg_direction_groups(int cnt, T &&...a)
{
  if (cnt >= 4)      mscg_direction_group<4, FIRST>(a...);
  else if (cnt == 3) mscg_direction_group<3, FIRST>(a...);
  else if (cnt == 2) mscg_direction_group<2, FIRST>(a...);
  else if (cnt == 1) mscg_direction_group<1, FIRST>(a...);
  else if (FIRST)    mscg_direction_group<0, FIRST>(a...);
}

__global__ __launch_bounds__(kRedThreads) void mscg_direction_kernel(int n, double *__restrict__ p, const double *__restrict__ r,
                                                                    double *P, long long ldp, const double *__restrict__ st,
                                                                    const double *__restrict__ ms)
{
  if (st[kStDone] != 0.0) return;
  const double beta = st[kStBeta];
  const int nb = __builtin_amdgcn_readfirstlane((int)st[kStNBase]), nl = __builtin_amdgcn_readfirstlane((int)st[kStNLive]);
  mscg_direction_groups<true>(nl, n, nb, beta, p, r, P, ldp, ms);
  for (int k0 = kMscgGroup; k0 < nl; k0 += kMscgGroup) mscg_direction_groups<false>(nl - k0, n, nb + k0, beta, p, r, P, ldp, ms);
}

// ---- fs_pcgn: (A'A + lambda I) X = B for k right-hand sides, k INDEPENDENT fs_pcg recurrences that share only the k-column products
// (include/fastsparse_hip.h spells the arithmetic out).  X, B, R, P, Q are row-major F x k panels.  st[] keeps done, the iteration
// count of the longest column and the mask of live columns; cs[] the per-column scalars, kPnStride doubles each.  Every per-column
// sum has fs_cg's tree over that column's F terms: row i belongs to thread (i / kRedThreads % kRedBlocks, i % kRedThreads), so a
// thread owns whole rows and keeps one (two: r.r and r.z) running sum per column in registers, KMAX columns at most.  The partials
// of sum v = column * ns + s (ns sums per column) are part[v * kRedBlocks + block]: the finisher reads them coalesced.
// A column that has converged is frozen: nothing writes its X, R or P again (its P rides through the products unchanged).  The
// columns of a row share cache lines, so a frozen column saves stores and arithmetic, not lines; only a tile of kPcgnTile columns
// (one 128-byte line per array) that are ALL frozen skips its loads: k > kPcgnTile only.
constexpr int kPcgnMaxRhs = FS_PCGN_MAX_RHS;
constexpr int kPcgnTile = 16;
constexpr int kPcgnRowsMaxK = 4;           // up to this k the lane-per-row kernels serve under "pcgn_kernel" = 0, beyond it the LDS-staged ones
enum { kStLiveMask = 12 };                 // bit j: column j is live (32 bits, exact in a double)
enum { kPnBb = 0, kPnRr = 1, kPnStop = 2, kPnRz = 3, kPnAlpha = 4, kPnBeta = 5, kPnCount = 6, kPnLive = 7, kPnConverged = 8,
       kPnStride = 16 };
static_assert(kCgStateLiveMask == kStLiveMask, "fs_common.h names the slot for the sharded solvers");
static_assert(kPcgnStateDoubles == kPcgnMaxRhs * kPnStride && pcgn_part_doubles(1) == (size_t)kRedBlocks * 2, "fs_common.h sizes the callers' buffers");
struct Pair { double a, b; };

// two neighbouring columns of a row: one 16-byte access (V: the address is 16-byte aligned, so k is even) or two of 8 bytes
template <bool V>
__device__ __forceinline__ Pair pn_ld(const double *p, bool two)
{
  if (V) { const double2 v = *reinterpret_cast<const double2 *>(p); return {v.x, v.y}; }
  return {p[0], two ? p[1] : 0.0};
}

template <bool V>
__device__ __forceinline__ void pn_st(double *p, Pair v, bool l0, bool l1)
{
  if (V && l0 && l1) { *reinterpret_cast<double2 *>(p) = make_double2(v.a, v.b); return; }
  if (l0) p[0] = v.a;
  if (l1) p[1] = v.b;
}

// the columns of a row that the lane-per-row kernels take together: at most kPcgnTile, one 128-byte line per array
template <int KMAX> constexpr int pcgn_tile() { return KMAX < kPcgnTile ? KMAX : kPcgnTile; }

// f(c0) for the tiles c0 = 0, tile, ... < k that hold a live column (wave-uniform branches; c0 is a constant once the loop is
// unrolled, so sums indexed by it stay in registers)
template <int KMAX, typename F>
__device__ __forceinline__ void pcgn_tiles(int k, unsigned live, F f)
{
  constexpr int T = pcgn_tile<KMAX>();
#pragma unroll
  for (int t = 0; t < KMAX / T; ++t)
    if (T * t < k && ((live >> (T * t)) & ((1u << T) - 1u)) != 0u) f(T * t);
}

// v[h] = the column pair c0 + 2 h of one array, for every pair of the tile.  A kernel calls this array by array before it computes
// or stores anything, so that all the 16-byte pieces a thread takes from a line are requested back to back (asked for one pair at
// a time, with stores in between, a line is evicted from the CU's 32 KB cache between its pieces)
template <int KMAX, bool V>
__device__ __forceinline__ void pcgn_ld_tile(Pair (&v)[pcgn_tile<KMAX>() / 2 + 1], const double *p, int c0, int k)
{
#pragma unroll
  for (int h = 0; h < pcgn_tile<KMAX>() / 2; ++h)
    if (c0 + 2 * h < k) v[h] = pn_ld<V>(p + c0 + 2 * h, c0 + 2 * h + 1 < k);
}

// g(h, c, column c is live, column c + 1 exists and is live) for the column pairs c = c0 + 2 h of a tile
template <int KMAX, typename G>
__device__ __forceinline__ void pcgn_tile_pairs(int c0, int k, unsigned live, G g)
{
#pragma unroll
  for (int h = 0; h < pcgn_tile<KMAX>() / 2; ++h) {
    const int c = c0 + 2 * h;
    if (c < k) g(h, c, ((live >> c) & 1u) != 0u, c + 1 < k && ((live >> (c + 1)) & 1u) != 0u);
  }
}

// ---- the per-column form of the kernels (fs_pcgn_lambdas).  LAM = PcgnLambdas in place of double: column c is shifted by
// lambda.v[c].  The kernels that see no lambda in fs_pcgn take the k lambdas as a trailing argument when the diagonal follows the
// column (FS_PRECOND_JACOBI): `dinv` then holds s = diag(A'A), and column c's inverse is formed per element, pcg_dinv_kernel's
// line on s + lambda_c.  The lambdas are a by-value argument, indexed by constants once the column loops are unrolled: scalar
// loads from the kernel's arguments, wave-uniform like al[c] and be[c].  Without LAM a kernel is fs_pcgn's own instantiation.
__device__ __forceinline__ double pn_inv(double s, double lambda)
{
  const double d = s + lambda;
  return d == 0.0 ? 1.0 : 1.0 / d;
}

// column c's lambda: the solve's one, one of the k by-value ones (lane-per-row kernels), one of the table in LDS (staged kernels)
__device__ __forceinline__ double pn_lambda(double lambda, int) { return lambda; }
__device__ __forceinline__ double pn_lambda(const PcgnLambdas &lambda, int c) { return lambda.v[c]; }
__device__ __forceinline__ double pn_lambda(const double *lam, int c) { return lam[c]; }

// a kernel's trailing LAM... as one value: the k lambdas, or PnOneDiag when the diagonal is the same for every column
struct PnOneDiag {};
__device__ __forceinline__ PnOneDiag pn_colj() { return {}; }
__device__ __forceinline__ const PcgnLambdas &pn_colj(const PcgnLambdas &lambda) { return lambda; }

// ---- the column steps: what one element of one column takes part in, each formula written here and nowhere else.  The
// lane-per-row kernels call them for the two columns of a Pair, the staged kernels column by column; a new per-column variant
// (another source of lambda, a weight) is added here.  Every product and sum rounds on its own, in this order (-ffp-contract=off)

// behind the product: q = q0 + l p, and q.p
__device__ __forceinline__ double pn_shift_dot(double q0, double l, double p, double &qp)
{
  const double q = q0 + l * p;
  qp += q * p;
  return q;
}

__device__ __forceinline__ double pn_x(double x0, double al, double p) { return x0 + al * p; }

// r = r0 - al q, and r.r
__device__ __forceinline__ double pn_r(double r0, double al, double q, double &rr)
{
  const double r = r0 - al * q;
  rr += r * r;
  return r;
}

// z of r: r without a preconditioner, r di with di = dinv[i], r / (di + lambda_c) with di = diag(A'A)[i] when the diagonal
// follows the column (pcg_dinv_kernel's line)
template <typename CJ>
__device__ __forceinline__ double pn_z(double r, bool pre, double di, const CJ &colj, int c)
{
  if constexpr (std::is_same<CJ, PnOneDiag>::value) return pre ? r * di : r;
  else return r * pn_inv(di, pn_lambda(colj, c));
}

__device__ __forceinline__ double pn_direction(double z, double be, double p0) { return z + be * p0; }

// the start: r = b, or warm q = q + l x, r = b - q; b.b and r.r
__device__ __forceinline__ double pn_init(bool warm, double &q, double l, double x, double b, double &bb, double &rr)
{
  if (warm) q = q + l * x;
  const double r = warm ? b - q : b;
  bb += b * b;
  rr += r * r;
  return r;
}

__device__ __forceinline__ unsigned pcgn_live(const double *__restrict__ st)
{
  return (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)st[kStLiveMask]);
}

// block_sum per live column: s0[c] (and s1[c] with ns = 2) over the workgroup -> part[(c * ns + s) * kRedBlocks + blockIdx]
template <int KMAX>
__device__ __forceinline__ void pcgn_block_sums(int k, unsigned live, int ns, const double (&s0)[KMAX], const double (&s1)[KMAX],
                                                double *__restrict__ part)
{
  __shared__ double sm[2 * KMAX][kRedThreads / 64];
#pragma unroll
  for (int c = 0; c < KMAX; ++c) {
    if (c < k && ((live >> c) & 1u) != 0u) {
      double s = s0[c];
      for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
      if ((threadIdx.x & 63) == 0) sm[2 * c][threadIdx.x >> 6] = s;
      if (ns == 2) {
        double z = s1[c];
        for (int m = 32; m > 0; m >>= 1) z += __shfl_xor(z, m);
        if ((threadIdx.x & 63) == 0) sm[2 * c + 1][threadIdx.x >> 6] = z;
      }
    }
  }
  __syncthreads();
  const int v = threadIdx.x, c = v / ns;
  if (v < ns * k && ((live >> c) & 1u) != 0u) {
    double s = 0.0;
    for (int w = 0; w < kRedThreads / 64; ++w) s += sm[2 * c + v % ns][w];
    part[(size_t)v * kRedBlocks + blockIdx.x] = s;
  }
}

// an array that the lane-per-row sweep loads: V as in pn_ld; not on: it is not read and its pairs are 0
template <bool V> struct PnArray { const double *p; bool on = true; };

// The lane-per-row sweep: a thread's rows in increasing order, of each row the tiles that hold a live column, of each tile the
// listed arrays loaded back to back (the comment above pcgn_ld_tile), then
// g(row * k, h, c, column c is live, column c + 1 is, dinv[row] or 1, v) for its column pairs c = c0 + 2 h: v[a][h] is the
// pair of the a-th array, and g stores what it changes
template <int KMAX, typename G, bool... V>
__device__ __forceinline__ void pcgn_rows(int n, int k, unsigned live, const double *dinv, G g, PnArray<V>... arr)
{
  for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) {
    const size_t row = (size_t)i * k;
    const double di = dinv ? dinv[i] : 1.0;
    pcgn_tiles<KMAX>(k, live, [&](int c0) {
      Pair v[sizeof...(V)][pcgn_tile<KMAX>() / 2 + 1] = {};
      int a = 0;
      ((arr.on ? pcgn_ld_tile<KMAX, V>(v[a++], arr.p + row, c0, k) : (void)a++), ...);
      pcgn_tile_pairs<KMAX>(c0, k, live, [&](int h, int c, bool l0, bool l1) { g(row, h, c, l0, l1, di, v); });
    });
  }
}

// cold: X = 0, R = B.  warm (Q = A'(A X) on entry): Q += lambda X, R = B - Q.  Partials {b.b, r.r} per column (pcg_init_kernel).
// VEC: 0 every access is 8 bytes (odd k), 1 16-byte accesses to the solve's own R, P, Q, 2 to the caller's X and B too
template <int KMAX, int VEC, typename LAM = double>
__global__ __launch_bounds__(kRedThreads) void pcgn_init_kernel(int n, int k, int warm, LAM lambda, const double *__restrict__ B,
                                                               double *__restrict__ X, double *__restrict__ R,
                                                               double *__restrict__ Q, double *__restrict__ part)
{
  double bb[KMAX], rr[KMAX];
#pragma unroll
  for (int c = 0; c < KMAX; ++c) { bb[c] = 0.0; rr[c] = 0.0; }
  const unsigned live = k < 32 ? (1u << k) - 1u : ~0u;
  pcgn_rows<KMAX>(n, k, live, nullptr, [&](size_t row, int h, int c, bool l0, bool l1, double, const auto &v) {
    const Pair b = v[0][h], x = v[1][h];
    Pair q = v[2][h];
    const Pair r = {pn_init(warm, q.a, pn_lambda(lambda, c), x.a, b.a, bb[c], rr[c]),
                    pn_init(warm, q.b, pn_lambda(lambda, c + 1), x.b, b.b, bb[c + 1], rr[c + 1])};
    if (warm) pn_st<VEC >= 1>(Q + row + c, q, l0, l1);
    else pn_st<VEC == 2>(X + row + c, {0.0, 0.0}, l0, l1);
    pn_st<VEC >= 1>(R + row + c, r, l0, l1);
  }, PnArray<VEC == 2>{B}, PnArray<VEC == 2>{X, warm != 0}, PnArray<VEC >= 1>{Q, warm != 0});
  pcgn_block_sums<KMAX>(k, live, 2, bb, rr, part);
}

// P = Z = R dinv (dinv != NULL) or R, partial r.z per live column (pcg_start_kernel).  Every column gets its first direction, the
// ones that are done at the start too: their P is finite when it rides through the products
template <int KMAX, int VEC, typename... LAM>
__global__ __launch_bounds__(kRedThreads) void pcgn_start_kernel(int n, int k, const double *__restrict__ R,
                                                                const double *__restrict__ dinv, double *__restrict__ P,
                                                                double *__restrict__ part, const double *__restrict__ st,
                                                                LAM... lambda)
{
  if (st[kStDone] != 0.0) return;
  const unsigned live = pcgn_live(st), all = k < 32 ? (1u << k) - 1u : ~0u;
  const auto &colj = pn_colj(lambda...);
  double rz[KMAX];
#pragma unroll
  for (int c = 0; c < KMAX; ++c) rz[c] = 0.0;
  pcgn_rows<KMAX>(n, k, all, dinv, [&](size_t row, int h, int c, bool l0, bool l1, double di, const auto &v) {
    const Pair r = v[0][h], z = {pn_z(r.a, dinv != nullptr, di, colj, c), pn_z(r.b, dinv != nullptr, di, colj, c + 1)};
    pn_st<VEC >= 1>(P + row + c, z, l0, l1);
    rz[c] += r.a * z.a; rz[c + 1] += r.b * z.b;
  }, PnArray<VEC >= 1>{R});
  pcgn_block_sums<KMAX>(k, live, 1, rz, rz, part);
}

// Q += lambda P, partial q.p per live column (cg_shift_dot_dev_kernel)
template <int KMAX, int VEC, typename LAM = double>
__global__ __launch_bounds__(kRedThreads) void pcgn_shift_dot_kernel(int n, int k, LAM lambda, double *__restrict__ Q,
                                                                    const double *__restrict__ P, double *__restrict__ part,
                                                                    const double *__restrict__ st)
{
  if (st[kStDone] != 0.0) return;
  const unsigned live = pcgn_live(st);
  double qp[KMAX];
#pragma unroll
  for (int c = 0; c < KMAX; ++c) qp[c] = 0.0;
  pcgn_rows<KMAX>(n, k, live, nullptr, [&](size_t row, int h, int c, bool l0, bool l1, double, const auto &v) {
    const Pair p = v[0][h], q0 = v[1][h];
    const Pair q = {pn_shift_dot(q0.a, pn_lambda(lambda, c), p.a, qp[c]), pn_shift_dot(q0.b, pn_lambda(lambda, c + 1), p.b, qp[c + 1])};
    pn_st<VEC >= 1>(Q + row + c, q, l0, l1);
  }, PnArray<VEC >= 1>{P}, PnArray<VEC >= 1>{Q});
  pcgn_block_sums<KMAX>(k, live, 1, qp, qp, part);
}

// per live column: x += alpha p, r -= alpha q, partial r.r; with a preconditioner z = r dinv and partial r.z in the same pass
// (pcg_update_kernel / cg_update_dev_kernel).  XUP false: r and its sums only, X is not touched (fs_mscgn: its x_ij have steps of their own)
template <int KMAX, int VEC, bool XUP, typename... LAM>
__global__ __launch_bounds__(kRedThreads) void pcgn_update_kernel(int n, int k, double *__restrict__ X, double *__restrict__ R,
                                                                 const double *__restrict__ P, const double *__restrict__ Q,
                                                                 const double *__restrict__ dinv, double *__restrict__ part,
                                                                 const double *__restrict__ st, const double *__restrict__ cs,
                                                                 LAM... lambda)
{
  if (st[kStDone] != 0.0) return;
  const unsigned live = pcgn_live(st);
  const auto &colj = pn_colj(lambda...);
  double rr[KMAX], rz[KMAX], al[KMAX];
#pragma unroll
  for (int c = 0; c < KMAX; ++c) { rr[c] = 0.0; rz[c] = 0.0; al[c] = cs[c * kPnStride + kPnAlpha]; }
  pcgn_rows<KMAX>(n, k, live, dinv, [&](size_t row, int h, int c, bool l0, bool l1, double di, const auto &v) {
    const Pair p = v[0][h], q = v[1][h], x0 = v[2][h], r0 = v[3][h];
    const Pair x = {pn_x(x0.a, al[c], p.a), pn_x(x0.b, al[c + 1], p.b)};
    const Pair r = {pn_r(r0.a, al[c], q.a, rr[c]), pn_r(r0.b, al[c + 1], q.b, rr[c + 1])};
    if (XUP) pn_st<VEC == 2>(X + row + c, x, l0, l1);
    pn_st<VEC >= 1>(R + row + c, r, l0, l1);
    if (sizeof...(LAM) != 0 || dinv) {
      rz[c] += r.a * pn_z(r.a, dinv != nullptr, di, colj, c); rz[c + 1] += r.b * pn_z(r.b, dinv != nullptr, di, colj, c + 1);
    }
  }, PnArray<VEC >= 1>{P}, PnArray<VEC >= 1>{Q}, PnArray<VEC == 2>{X, XUP}, PnArray<VEC >= 1>{R});
  pcgn_block_sums<KMAX>(k, live, dinv ? 2 : 1, rr, rz, part);
}

// per live column: p = z + beta p with z = r dinv formed on the fly, or p = r + beta p (pcg_direction_kernel / cg_direction_dev_kernel)
template <int KMAX, int VEC, typename... LAM>
__global__ __launch_bounds__(kRedThreads) void pcgn_direction_kernel(int n, int k, double *__restrict__ P, const double *__restrict__ R,
                                                                    const double *__restrict__ dinv, const double *__restrict__ st,
                                                                    const double *__restrict__ cs, LAM... lambda)
{
  if (st[kStDone] != 0.0) return;
  const unsigned live = pcgn_live(st);
  const auto &colj = pn_colj(lambda...);
  double be[KMAX];
#pragma unroll
  for (int c = 0; c < KMAX; ++c) be[c] = cs[c * kPnStride + kPnBeta];
  pcgn_rows<KMAX>(n, k, live, dinv, [&](size_t row, int h, int c, bool l0, bool l1, double di, const auto &v) {
    const Pair r = v[0][h], p0 = v[1][h];
    const Pair z = {pn_z(r.a, dinv != nullptr, di, colj, c), pn_z(r.b, dinv != nullptr, di, colj, c + 1)};
    const Pair p = {pn_direction(z.a, be[c], p0.a), pn_direction(z.b, be[c + 1], p0.b)};
    pn_st<VEC >= 1>(P + row + c, p, l0, l1);
  }, PnArray<VEC >= 1>{R}, PnArray<VEC >= 1>{P});
}

// ---- the per-iteration kernels again, the panels staged through LDS (option "pcgn_kernel" = 2; auto for k > kPcgnRowsMaxK).  A
// workgroup's 256 rows of a row-major panel are one contiguous piece of 256 k doubles: it is read with coalesced 16-byte loads
// (every line touched once, by neighbouring lanes) into a tile of LDS padded to an odd row length, where every thread then works on
// its own row without bank conflicts, and goes back the same way.  Two tiles: the array that is updated and the one it is updated
// with.  Row i still belongs to thread (i / 256 % 1024, i % 256) and a thread still adds its
// rows' terms in increasing order to sums in registers: the same tree, the same bits.  Nothing is skipped for frozen columns but
// their arithmetic and their stores (a column's doubles share every line with its neighbours').
// rows of a tile: all 256 of the workgroup up to KMAX = 8, then fewer, so that the two tiles stay at 35 KB and four workgroups share
// a CU (with 256 rows at KMAX = 32 -- 135 KB, one workgroup per CU, loading, computing and storing in turn -- the kernels reached
// 2.1 TB/s where the lane-per-row kernels reach 2.7)
template <int KMAX> constexpr int pl_rows() { return KMAX <= 8 ? kRedThreads : kRedThreads * 8 / KMAX; }

template <int KMAX>
__device__ __forceinline__ void pl_in(double *__restrict__ tile, const double *__restrict__ g, int ne, int k)
{
  constexpr int LD = KMAX + 1;
  if (((uintptr_t)g & 15) == 0) {
#pragma unroll 4
    for (int e = 2 * threadIdx.x; e < ne; e += 2 * kRedThreads) {
      const int r = e / k, c = e - r * k;
      if (e + 1 < ne) {
        const double2 d = *reinterpret_cast<const double2 *>(g + e);
        tile[r * LD + c] = d.x;
        tile[c + 1 < k ? r * LD + c + 1 : (r + 1) * LD] = d.y;
      } else {
        tile[r * LD + c] = g[e];
      }
    }
  } else {
#pragma unroll 4
    for (int e = threadIdx.x; e < ne; e += kRedThreads) {
      const int r = e / k;
      tile[r * LD + e - r * k] = g[e];
    }
  }
}

// the live columns of the tile back to the panel (a frozen column is not written)
template <int KMAX>
__device__ __forceinline__ void pl_out(double *__restrict__ g, const double *__restrict__ tile, int ne, int k, unsigned live)
{
  constexpr int LD = KMAX + 1;
  if (((uintptr_t)g & 15) == 0) {
    for (int e = 2 * threadIdx.x; e < ne; e += 2 * kRedThreads) {
      const int r = e / k, c = e - r * k;
      const bool two = e + 1 < ne;
      const int c1 = c + 1 < k ? c + 1 : 0;
      const double a = tile[r * LD + c], b = two ? tile[c + 1 < k ? r * LD + c + 1 : (r + 1) * LD] : 0.0;
      const bool l0 = ((live >> c) & 1u) != 0u, l1 = two && ((live >> c1) & 1u) != 0u;
      if (l0 && l1) *reinterpret_cast<double2 *>(g + e) = make_double2(a, b);
      else if (l0) g[e] = a;
      else if (l1) g[e + 1] = b;
    }
  } else {
    for (int e = threadIdx.x; e < ne; e += kRedThreads) {
      const int r = e / k, c = e - r * k;
      if (((live >> c) & 1u) != 0u) g[e] = tile[r * LD + c];
    }
  }
}

// the staged kernels of the per-column form keep the k lambdas in LDS: a lane reads lam[c] as a broadcast, and no scalar registers
// are held across the tile loop (with the lambdas in SGPRs the shift-dot kernel at KMAX = 32 went from 128 to 130 VGPRs, from four
// waves per SIMD to three and from 1.6 to 2.7 ms).  Read behind the tile loop's first barrier.  What pn_lambda and pn_z take in a
// staged kernel: that table for the k lambdas, the one lambda and no lambda as they are
template <int KMAX>
__device__ __forceinline__ const double *pl_lambdas(const PcgnLambdas &lambda)
{
  __shared__ double lam[KMAX];
  if (threadIdx.x < KMAX) lam[threadIdx.x] = lambda.v[threadIdx.x];
  return lam;
}
template <int KMAX> __device__ __forceinline__ double pl_lambdas(double lambda) { return lambda; }
template <int KMAX> __device__ __forceinline__ PnOneDiag pl_lambdas() { return {}; }

// The staged sweep: the workgroup's rows, 256 per grid stride and TR of them at a time, and for each such piece f(pass).
// pass(A, B, dinv, col) is one trip through LDS: the piece of A and of B in, the thread that owns a row sets
// a[c] = col(c, a[c], b[c], dinv[row] or 1) for its live columns, A's live columns out
template <int KMAX, typename F>
__device__ __forceinline__ void pl_sweep(int n, int k, unsigned live, F f)
{
  constexpr int LD = KMAX + 1;
  constexpr int TR = pl_rows<KMAX>();
  __shared__ double t0[TR * LD], t1[TR * LD];
  for (int blk0 = blockIdx.x * kRedThreads; blk0 < n; blk0 += gridDim.x * kRedThreads)      // (workgroup-uniform)
  for (int row0 = blk0; row0 < blk0 + kRedThreads && row0 < n; row0 += TR) {                // the workgroup's 256 rows, TR at a time
    const int nr = n - row0 < TR ? n - row0 : TR, ne = nr * k, lt = (int)threadIdx.x - (row0 - blk0);
    const size_t at = (size_t)row0 * k;
    f([&](double *A, const double *B, const double *dinv, auto col) {
      pl_in<KMAX>(t0, A + at, ne, k);
      pl_in<KMAX>(t1, B + at, ne, k);
      __syncthreads();
      if (lt >= 0 && lt < nr) {                               // the thread that owns row row0 + lt
        double *a = t0 + lt * LD;
        const double *b = t1 + lt * LD;
        const double di = dinv ? dinv[row0 + lt] : 1.0;
#pragma unroll
        for (int c = 0; c < KMAX; ++c)
          if (c < k && ((live >> c) & 1u) != 0u) a[c] = col(c, a[c], b[c], di);
      }
      __syncthreads();
      pl_out<KMAX>(A + at, t0, ne, k, live);
      __syncthreads();
    });
  }
}

// Q += lambda P, partial q.p per live column
template <int KMAX, typename LAM = double>
__global__ __launch_bounds__(kRedThreads) void pcgn_shift_dot_lds_kernel(int n, int k, LAM lambda, double *__restrict__ Q,
                                                                        const double *__restrict__ P, double *__restrict__ part,
                                                                        const double *__restrict__ st)
{
  if (st[kStDone] != 0.0) return;
  const auto lam = pl_lambdas<KMAX>(lambda);
  const unsigned live = pcgn_live(st);
  double qp[KMAX];
#pragma unroll
  for (int c = 0; c < KMAX; ++c) qp[c] = 0.0;
  pl_sweep<KMAX>(n, k, live, [&](auto pass) {
    pass(Q, P, nullptr, [&](int c, double q0, double p, double) { return pn_shift_dot(q0, pn_lambda(lam, c), p, qp[c]); });
  });
  pcgn_block_sums<KMAX>(k, live, 1, qp, qp, part);
}

// per live column: x += alpha p (XUP), then r -= alpha q with the partials of r.r and, with a preconditioner, of r.z (z = r dinv)
template <int KMAX, bool XUP, typename... LAM>
__global__ __launch_bounds__(kRedThreads) void pcgn_update_lds_kernel(int n, int k, double *__restrict__ X, double *__restrict__ R,
                                                                     const double *__restrict__ P, const double *__restrict__ Q,
                                                                     const double *__restrict__ dinv, double *__restrict__ part,
                                                                     const double *__restrict__ st, const double *__restrict__ cs,
                                                                     LAM... lambda)
{
  if (st[kStDone] != 0.0) return;
  const auto colj = pl_lambdas<KMAX>(lambda...);
  const unsigned live = pcgn_live(st);
  double rr[KMAX], rz[KMAX], al[KMAX];
#pragma unroll
  for (int c = 0; c < KMAX; ++c) { rr[c] = 0.0; rz[c] = 0.0; al[c] = cs[c * kPnStride + kPnAlpha]; }
  pl_sweep<KMAX>(n, k, live, [&](auto pass) {
    if (XUP) pass(X, P, nullptr, [&](int c, double x0, double p, double) { return pn_x(x0, al[c], p); });
    pass(R, Q, dinv, [&](int c, double r0, double q, double di) {
      const double r = pn_r(r0, al[c], q, rr[c]);
      if (sizeof...(LAM) != 0 || dinv) rz[c] += r * pn_z(r, dinv != nullptr, di, colj, c);
      return r;
    });
  });
  pcgn_block_sums<KMAX>(k, live, dinv ? 2 : 1, rr, rz, part);
}

// per live column: p = z + beta p with z = r dinv formed on the fly, or p = r + beta p
template <int KMAX, typename... LAM>
__global__ __launch_bounds__(kRedThreads) void pcgn_direction_lds_kernel(int n, int k, double *__restrict__ P, const double *__restrict__ R,
                                                                        const double *__restrict__ dinv, const double *__restrict__ st,
                                                                        const double *__restrict__ cs, LAM... lambda)
{
  if (st[kStDone] != 0.0) return;
  const auto colj = pl_lambdas<KMAX>(lambda...);
  const unsigned live = pcgn_live(st);
  double be[KMAX];
#pragma unroll
  for (int c = 0; c < KMAX; ++c) be[c] = cs[c * kPnStride + kPnBeta];
  pl_sweep<KMAX>(n, k, live, [&](auto pass) {
    pass(P, R, dinv, [&](int c, double p0, double r, double di) { return pn_direction(pn_z(r, dinv != nullptr, di, colj, c), be[c], p0); });
  });
}

// stage 2 of the ns sums of every live column, kPcgnGroup sums' loads in flight together: sum v = column * ns + s is fs_cg's stage 2
// over its kRedBlocks partials part[v * kRedBlocks + b], or (RANKS: the slice sums of `count` ranks, gathered, rank b's nv values at
// b * nv) over the ranks' values in rank order.  Leaves the waves' sums in sm[v][]; a frozen column's are +0.0
constexpr int kPcgnGroup = 8;
template <bool RANKS>
__device__ __forceinline__ void pcgn_fold(const double *__restrict__ part, int count, unsigned live, int nv, int ns,
                                          double (&sm)[2 * kPcgnMaxRhs][kRedThreads / 64])
{
  for (int v0 = 0; v0 < nv; v0 += kPcgnGroup) {
    double a[kPcgnGroup];
#pragma unroll
    for (int u = 0; u < kPcgnGroup; ++u) {
      const int v = v0 + u;
      a[u] = 0.0;
      if (v < nv && ((live >> (v / ns)) & 1u) != 0u) {
        if (RANKS) for (int b = threadIdx.x; b < count; b += kRedThreads) a[u] += part[(size_t)b * nv + v];
        else for (int b = threadIdx.x; b < kRedBlocks; b += kRedThreads) a[u] += part[(size_t)v * kRedBlocks + b];
      }
    }
#pragma unroll
    for (int u = 0; u < kPcgnGroup; ++u) {
      double s = a[u];
      for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
      if ((threadIdx.x & 63) == 0 && v0 + u < nv) sm[v0 + u][threadIdx.x >> 6] = s;
    }
  }
}

// a rank's slice sums into its send slot (fs_dist_pcgn_lambdas, fs_dist_mscgn on slices): one workgroup, the first half of
// pcgn_step_kernel.  `start`: every column is live (behind pcgn_init_kernel).  A frozen column's slots are sent as +0.0.
// ranks > 0: `part` holds the gathered slots of that many ranks (rank r's ns * k values at r * ns * k), added in rank order into
// send[] -- the first half of pcgn_step_kernel<STEP, true>, for a scalar step that is a kernel of its own (fs_dist_mscgn:
// mscgn_step_kernel)
__global__ __launch_bounds__(kRedThreads) void pcgn_fold_kernel(const double *__restrict__ part, int ranks, double *__restrict__ send,
                                                               const double *__restrict__ st, int k, int ns, int start)
{
  if (!start && st[kStDone] != 0.0) return;
  __shared__ double sm[2 * kPcgnMaxRhs][kRedThreads / 64];
  const unsigned live = start ? (k < 32 ? (1u << k) - 1u : ~0u) : pcgn_live(st);
  const int nv = ns * k;
  if (ranks > 0) pcgn_fold<true>(part, ranks, live, nv, ns, sm);         // (a kernel argument: uniform)
  else pcgn_fold<false>(part, kRedBlocks, live, nv, ns, sm);
  __syncthreads();
  if ((int)threadIdx.x < nv) {
    double s = 0.0;
    for (int w = 0; w < kRedThreads / 64; ++w) s += sm[threadIdx.x][w];
    send[threadIdx.x] = s;
  }
}

// the one workgroup that finishes the ns sums of every live column (pcgn_fold: over the kRedBlocks partials of whole panels, or
// RANKS: over the gathered slice sums of `count` ranks) and then does the scalar step of fs_pcg per column, one thread each
// (final_step_kernel's kStepPcgStart, kStepPcgRz, kStepCgAlpha, kStepPcgBeta with `done` per column); thread 0 then packs the live
// mask.  done: no column is live; st[kStIter] counts the iterations after which a column was still live (the longest column's
// count).  With RANKS every rank runs this over the same gathered values: identical scalars, freezes and masks everywhere
template <PcgnStep STEP, bool RANKS = false>
__global__ __launch_bounds__(kRedThreads) void pcgn_step_kernel(const double *__restrict__ part, int count, double *st, double *cs, int k,
                                                               int ns, double tol)
{
  if (STEP != kPnStepStart && st[kStDone] != 0.0) return;
  __shared__ double sm[2 * kPcgnMaxRhs][kRedThreads / 64];
  __shared__ double red[2 * kPcgnMaxRhs];
  const unsigned live = STEP == kPnStepStart ? (k < 32 ? (1u << k) - 1u : ~0u) : pcgn_live(st);
  const int nv = ns * k;
  pcgn_fold<RANKS>(part, count, live, nv, ns, sm);
  __syncthreads();
  if ((int)threadIdx.x < nv) {
    double s = 0.0;
    for (int w = 0; w < kRedThreads / 64; ++w) s += sm[threadIdx.x][w];
    red[threadIdx.x] = s;
  }
  __syncthreads();
  const int c = threadIdx.x;
  if (c < k && ((live >> c) & 1u) != 0u) {
    double *e = cs + c * kPnStride;
    const double s0 = red[c * ns], s1 = red[c * ns + ns - 1];
    if (STEP == kPnStepStart) {                              // {b.b, r.r}
      const double stop = tol * sqrt(s0);
      const bool done = sqrt(s1) <= stop;
      e[kPnBb] = s0; e[kPnRr] = s1; e[kPnStop] = stop; e[kPnCount] = 0.0;
      e[kPnLive] = done ? 0.0 : 1.0; e[kPnConverged] = done ? 1.0 : 0.0;
    } else if (STEP == kPnStepRz) {
      e[kPnRz] = s0;
    } else if (STEP == kPnStepAlpha) {                       // q.p
      e[kPnAlpha] = e[kPnRz] / s0;
    } else {                                                 // {r.r[, r.z]}
      const double rr = s0, rz_new = s1;
      e[kPnRr] = rr;
      if (sqrt(rr) <= e[kPnStop]) { e[kPnLive] = 0.0; e[kPnConverged] = 1.0; }
      else { e[kPnBeta] = rz_new / e[kPnRz]; e[kPnRz] = rz_new; e[kPnCount] += 1.0; }
    }
  }
  if (STEP != kPnStepStart && STEP != kPnStepBeta) return;
  __syncthreads();
  if (threadIdx.x != 0) return;
  unsigned m = 0u;
  for (int j = 0; j < k; ++j)
    if (cs[j * kPnStride + kPnLive] != 0.0) m |= 1u << j;
  st[kStLiveMask] = (double)m;
  if (STEP == kPnStepStart) { st[kStIter] = 0.0; st[kStDone] = m ? 0.0 : 1.0; }
  else if (m == 0u) st[kStDone] = 1.0;
  else st[kStIter] += 1.0;
}

// ---- option "pcgn_compact": the live columns of a solve move into a narrower panel (the schedule: fs_pcgn_plan.h).  One launch
// takes up to three row-major n x ws panels (X, R, P) to three n x wd panels: destination column c is source column map.v[c], or,
// where map.v[c] < 0, +0.0 (KEEP false: a padding column of the narrower panel) or left as it is (KEEP true: the way back, the
// finished columns of a narrow X into the caller's n x k panel, whose other columns belong to other recurrences).  A pure stream
// in the shape of the staged vector kernels: the workgroup's 256 rows, pl_rows at a time, come in with coalesced 16-byte loads
// into a tile of LDS padded to an odd row length and leave in destination order with coalesced 16-byte stores; the 1024 x 256
// grid with a grid stride.  tiles: bit t set when a column 16 t .. 16 t + 15 of the source is selected -- a 16-column tile (one
// 128-byte line of an aligned row) without a selected column is not loaded.  st != NULL: a launch behind the end of the solve
// does nothing, like the iteration it was enqueued with.
struct PcgnColMap { signed char v[kPcgnMaxRhs]; };

template <int KMAX>
__device__ __forceinline__ void pr_in(double *__restrict__ tile, const double *__restrict__ g, int ne, int k, unsigned tiles)
{
  constexpr int LD = KMAX + 1;
  if (((uintptr_t)g & 15) == 0) {
#pragma unroll 4
    for (int e = 2 * threadIdx.x; e < ne; e += 2 * kRedThreads) {
      const int r = e / k, c = e - r * k, c1 = c + 1 < k ? c + 1 : 0;
      if ((((tiles >> (c >> 4)) | (tiles >> (c1 >> 4))) & 1u) == 0u) continue;
      if (e + 1 < ne) {
        const double2 d = *reinterpret_cast<const double2 *>(g + e);
        tile[r * LD + c] = d.x;
        tile[c + 1 < k ? r * LD + c + 1 : (r + 1) * LD] = d.y;
      } else {
        tile[r * LD + c] = g[e];
      }
    }
  } else {
#pragma unroll 4
    for (int e = threadIdx.x; e < ne; e += kRedThreads) {
      const int r = e / k, c = e - r * k;
      if (((tiles >> (c >> 4)) & 1u) != 0u) tile[r * LD + c] = g[e];
    }
  }
}

// ne = rows x wd doubles of the destination, from the tile's columns smap[c]
template <int KMAX, bool KEEP>
__device__ __forceinline__ void pr_out(double *__restrict__ g, const double *__restrict__ tile, int ne, int wd, const int *__restrict__ smap)
{
  constexpr int LD = KMAX + 1;
  if (((uintptr_t)g & 15) == 0) {
    for (int e = 2 * threadIdx.x; e < ne; e += 2 * kRedThreads) {
      const int r = e / wd, c = e - r * wd;
      const bool two = e + 1 < ne;
      const int r1 = c + 1 < wd ? r : r + 1, c1 = c + 1 < wd ? c + 1 : 0;
      const int s0 = smap[c], s1 = two ? smap[c1] : -1;
      const double a = s0 >= 0 ? tile[r * LD + s0] : 0.0, b = s1 >= 0 ? tile[r1 * LD + s1] : 0.0;
      const bool w0 = !KEEP || s0 >= 0, w1 = two && (!KEEP || s1 >= 0);
      if (w0 && w1) *reinterpret_cast<double2 *>(g + e) = make_double2(a, b);
      else if (w0) g[e] = a;
      else if (w1) g[e + 1] = b;
    }
  } else {
    for (int e = threadIdx.x; e < ne; e += kRedThreads) {
      const int r = e / wd, s0 = smap[e - r * wd];
      if (!KEEP || s0 >= 0) g[e] = s0 >= 0 ? tile[r * LD + s0] : 0.0;
    }
  }
}

// KMAX: the shape of the source width (ws <= KMAX)
template <int KMAX, bool KEEP>
__global__ __launch_bounds__(kRedThreads) void pcgn_repack_kernel(int n, int ws, int wd, PcgnColMap map, unsigned tiles,
                                                                 const double *__restrict__ S0, const double *__restrict__ S1,
                                                                 const double *__restrict__ S2, double *__restrict__ D0,
                                                                 double *__restrict__ D1, double *__restrict__ D2,
                                                                 const double *__restrict__ st)
{
  if (st && st[kStDone] != 0.0) return;
  constexpr int LD = KMAX + 1;
  constexpr int TR = pl_rows<KMAX>();
  __shared__ double t0[TR * LD];
  __shared__ int smap[kPcgnMaxRhs];
  if (threadIdx.x < kPcgnMaxRhs) smap[threadIdx.x] = map.v[threadIdx.x];   // (read behind the tile loop's first barrier)
  for (int blk0 = blockIdx.x * kRedThreads; blk0 < n; blk0 += gridDim.x * kRedThreads)      // (workgroup-uniform)
  for (int row0 = blk0; row0 < blk0 + kRedThreads && row0 < n; row0 += TR) {                // the workgroup's 256 rows, TR at a time
    const int nr = n - row0 < TR ? n - row0 : TR;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double *S = a == 0 ? S0 : a == 1 ? S1 : S2;
      double *D = a == 0 ? D0 : a == 1 ? D1 : D2;
      if (!S) continue;                                                                     // (a kernel argument: uniform)
      pr_in<KMAX>(t0, S + (size_t)row0 * ws, nr * ws, ws, tiles);
      __syncthreads();
      pr_out<KMAX, KEEP>(D + (size_t)row0 * wd, t0, nr * wd, wd, smap);
      __syncthreads();
    }
  }
}

// the scalars follow their columns: one workgroup.  cs[] holds the w_old columns of the panel the solve leaves, home[] every
// column's scalars in ORIGINAL numbering.  First the columns of the old panel go home (home_of.v[c]: the original column of the
// old panel's column c, < 0: padding) -- a column that stays behind is final there.  Then cs[] and st[kStLiveMask] are rewritten
// for the new panel: its column c is the old panel's column from.v[c]; from.v[c] < 0: padding, all zeros, not live.  k_final > 0
// (the end of the solve) instead leaves the mask of the k_final original columns in st[]: home[] is then the solve's cs[]
__global__ __launch_bounds__(kRedThreads) void pcgn_remap_kernel(double *st, double *cs, double *home, PcgnColMap home_of, PcgnColMap from,
                                                                int w_old, int w_new, int k_final, int check_done)
{
  if (check_done && st[kStDone] != 0.0) return;
  __shared__ double a[kPcgnMaxRhs * kPnStride];
  __shared__ int ho[kPcgnMaxRhs], fr[kPcgnMaxRhs];
  for (int i = threadIdx.x; i < kPcgnMaxRhs * kPnStride; i += kRedThreads) a[i] = i < w_old * kPnStride ? cs[i] : 0.0;
  if (threadIdx.x < kPcgnMaxRhs) { ho[threadIdx.x] = home_of.v[threadIdx.x]; fr[threadIdx.x] = from.v[threadIdx.x]; }
  __syncthreads();
  for (int i = threadIdx.x; i < w_old * kPnStride; i += kRedThreads) {
    const int o = ho[i / kPnStride];
    if (o >= 0) home[o * kPnStride + i % kPnStride] = a[i];
  }
  if (k_final > 0) {
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned m = 0u;
    for (int j = 0; j < k_final; ++j)
      if (home[j * kPnStride + kPnLive] != 0.0) m |= 1u << j;
    st[kStLiveMask] = (double)m;
    return;
  }
  for (int i = threadIdx.x; i < kPcgnMaxRhs * kPnStride; i += kRedThreads) {
    const int c = i / kPnStride, s = c < w_new ? fr[c] : -1;
    cs[i] = s >= 0 ? a[s * kPnStride + i % kPnStride] : 0.0;
  }
  if (threadIdx.x != 0) return;
  unsigned m = 0u;
  for (int c = 0; c < w_new; ++c)
    if (fr[c] >= 0 && a[fr[c] * kPnStride + kPnLive] != 0.0) m |= 1u << c;
  st[kStLiveMask] = (double)m;
}

// ---- fs_mscgn: fs_mscg on every column of a row-major F x k panel B, m lambdas shared by all columns, on ONE pair of k-column
// products per iteration (include/fastsparse_hip.h says what differs from fs_mscg).  Column j has fs_mscg's scalars to itself:
// cst[j * kStDoubles ..] in the layout of fs_mscg's st[], ms[j * kMscgStateDoubles ..] in that of its ms[], and the scalar steps
// ARE fs_mscg's (mscg_start_step, mscg_s1_step, mscg_s2_step), one column per kMscgMaxShifts threads.  The per-column sums are
// fs_pcgn's: its kernels form q + base p with q.p and r - alpha q with r.r (pcgn_update_kernel without its X), pcgn_fold_kernel
// finishes them, so st[] carries fs_pcgn's done, iteration count and mask of live columns and cs[] column j's alpha where those
// kernels read it.  What fs_mscg does per shift runs per PAIR (shift i, column j) here and needs no sum: x_ij += a_ij P_ij and
// P_ij = z_ij r_j + b_ij P_ij stream the row-major panels flat -- element e of a panel belongs to column e % k, whose coefficient
// comes from a table in LDS -- fully coalesced, 16 bytes at a time where k is even and the panel is 16-byte aligned.
// sl[]: what the flat kernels need per SHIFT -- the compacted list of the shifts that still have a live pair (sigma = 0 first, then
// the others, in the caller's order: kSlNBase + kSlNLive entries), every shift's mask of live columns and its direction slot.
constexpr int kMscgnColumnsPerPass = kRedThreads / kMscgMaxShifts;
enum { kSlNBase = 0, kSlNLive = 1, kSlList = 2, kSlMask = kSlList + kMscgMaxShifts, kSlPslot = kSlMask + kMscgMaxShifts, kSlDoubles = 64 };
static_assert(kSlPslot + kMscgMaxShifts <= kSlDoubles && kSlDoubles == kMscgnListDoubles, "fs_common.h sizes sl[]");
static_assert(kMscgnColumnsPerPass * kMscgMaxShifts == kRedThreads && kMscgGroup * kPcgnMaxRhs <= kRedThreads, "one thread per pair and per table entry");

// the one-workgroup step behind the k finished sums red[j * ns] (pcgn_fold_kernel's): fs_mscg's scalar step for every live column,
// one thread per pair, kMscgnColumnsPerPass columns at a time; then (start, S2) the masks and the list of sl[] and fs_pcgn's mask of
// live columns.  A column is live while its fs_mscg is not done; done: no column is live
template <MscgStep STEP>
__global__ __launch_bounds__(kRedThreads) void mscgn_step_kernel(const double *__restrict__ red, double *st, double *cst, double *cs,
                                                                double *ms, double *sl, int k, int m, double tol, MscgSigma sg)
{
  if (STEP != kMscgStart && st[kStDone] != 0.0) return;
  const unsigned live = STEP == kMscgStart ? (k < 32 ? (1u << k) - 1u : ~0u) : pcgn_live(st);
  const int ns = STEP == kMscgStart ? 2 : 1;                 // {b.b, r.r} behind pcgn_init_kernel
  const int lane = threadIdx.x % kMscgMaxShifts;
  for (int j0 = 0; j0 < k; j0 += kMscgnColumnsPerPass) {       // (workgroup-uniform: the steps hold barriers)
    const int j = j0 + threadIdx.x / kMscgMaxShifts;
    const bool active = j < k && ((live >> j) & 1u) != 0u;
    const int ja = j < k ? j : 0;
    double *stj = cst + ja * kStDoubles, *msj = ms + ja * kMscgStateDoubles;
    const double *rj = red + ja * ns;
    if (STEP == kMscgStart) {
      mscg_start_step(rj[0], tol, stj, msj, m, sg, lane, active);
    } else if (STEP == kMscgS1) {
      mscg_s1_step(rj, stj, msj, m, lane, active);
      if (active && lane == 0) cs[j * kPnStride + kPnAlpha] = stj[kStAlpha];
    } else {
      mscg_s2_step(rj, stj, msj, m, lane, active);
    }
  }
  if (STEP == kMscgS1) return;
  __syncthreads();
  if ((int)threadIdx.x < m) {                                // per shift: the columns whose pair is live
    unsigned mk = 0u;
    for (int j = 0; j < k; ++j)
      if (cst[j * kStDoubles + kStDone] == 0.0 && ms[j * kMscgStateDoubles + threadIdx.x * kMsStride + kMsLive] != 0.0) mk |= 1u << j;
    sl[kSlMask + threadIdx.x] = (double)mk;
    if (STEP == kMscgStart) sl[kSlPslot + threadIdx.x] = ms[threadIdx.x * kMsStride + kMsPslot];   // (the same in every column)
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  unsigned cm = 0u;
  for (int j = 0; j < k; ++j)
    if (cst[j * kStDoubles + kStDone] == 0.0) cm |= 1u << j;
  int nb = 0, nl = 0;
  for (int i = 0; i < m; ++i)
    if (sl[kSlMask + i] != 0.0 && sg.v[i] == 0.0) sl[kSlList + nb++] = (double)i;
  for (int i = 0; i < m; ++i)
    if (sl[kSlMask + i] != 0.0 && sg.v[i] != 0.0) sl[kSlList + nb + nl++] = (double)i;
  sl[kSlNBase] = (double)nb; sl[kSlNLive] = (double)nl;
  st[kStLiveMask] = (double)cm;
  if (STEP == kMscgStart) { st[kStIter] = 0.0; st[kStDone] = cm ? 0.0 : 1.0; }
  else if (cm == 0u) st[kStDone] = 1.0;
  else st[kStIter] += 1.0;
}

// one (V: two neighbouring, e even and k even, so both in one row) element of a panel streamed flat; al: 16-byte aligned panel
template <bool V>
__device__ __forceinline__ Pair fl_ld(const double *p, bool al)
{
  if (V && al) return pn_ld<true>(p, true);
  return pn_ld<false>(p, V);
}

template <bool V>
__device__ __forceinline__ void fl_st(double *p, Pair v, bool al, bool l0, bool l1)
{
  if (V && al) pn_st<true>(p, v, l0, V && l1);
  else pn_st<false>(p, v, l0, V && l1);
}

__device__ __forceinline__ bool fl_aligned(const double *p) { return ((uintptr_t)p & 15) == 0; }

// what fs_pcgn's start leaves to do: P = B, P_i = B for the nslots shifts with sigma != 0, X_i = 0 for the shifts behind the first
// (pcgn_init_kernel wrote X_0 = 0 and R = B)
template <bool V>
__global__ __launch_bounds__(kRedThreads) void mscgn_fill_kernel(size_t ne, const double *__restrict__ B, double *__restrict__ P,
                                                                double *__restrict__ Ps, size_t ldp, int nslots, double *__restrict__ X,
                                                                size_t ldx, int m)
{
  constexpr int W = V ? 2 : 1;
  const bool ba = fl_aligned(B);
  for (size_t e = ((size_t)blockIdx.x * kRedThreads + threadIdx.x) * W; e < ne; e += (size_t)gridDim.x * kRedThreads * W) {
    const Pair b = fl_ld<V>(B + e, ba);
    fl_st<V>(P + e, b, true, true, true);
    for (int s = 0; s < nslots; ++s) fl_st<V>(Ps + s * ldp + e, b, true, true, true);
    for (int i = 1; i < m; ++i) fl_st<V>(X + i * ldx + e, {0.0, 0.0}, fl_aligned(X + i * ldx), true, true);
  }
}

// the shifts of one group: their place in the list -> panel of X, direction (P itself for sigma = 0), mask of live columns
struct MscgnShift { double *x; const double *p; double *pw; unsigned mask; bool xa; };
__device__ __forceinline__ MscgnShift mscgn_shift(const double *__restrict__ sl, int at, double *X, size_t ldx, const double *P, double *Ps,
                                                  size_t ldp)
{
  const int sh = __builtin_amdgcn_readfirstlane((int)sl[kSlList + at]);
  const int slot = __builtin_amdgcn_readfirstlane((int)sl[kSlPslot + sh]);
  const unsigned mask = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)sl[kSlMask + sh]);
  double *x = X ? X + sh * ldx : nullptr;
  double *pw = slot < 0 ? nullptr : Ps + slot * ldp;
  return {x, slot < 0 ? P : pw, pw, mask, fl_aligned(x)};
}

// x_ij = x_ij + a_ij P_ij for the live pairs of CNT shifts (their loads in flight together); co[u][c]: a of the group's shift u in
// column c.  A frozen pair is not written
template <int CNT, bool V>
__device__ __forceinline__ void mscgn_update_group(size_t ne, int k, int at, double *X, size_t ldx, const double *P, double *Ps, size_t ldp,
                                                   const double *__restrict__ sl, const double (&co)[kMscgGroup][kPcgnMaxRhs])
{
  constexpr int W = V ? 2 : 1;
  MscgnShift g[CNT + 1];
#pragma unroll
  for (int u = 0; u < CNT; ++u) g[u] = mscgn_shift(sl, at + u, X, ldx, P, Ps, ldp);
  const size_t stride = (size_t)gridDim.x * kRedThreads * W;
  size_t e = ((size_t)blockIdx.x * kRedThreads + threadIdx.x) * W;
  int c = (int)(e % (size_t)k);
  const int cstep = (int)(stride % (size_t)k);
  for (; e < ne; e += stride) {
    Pair pv[CNT + 1], xv[CNT + 1];
#pragma unroll
    for (int u = 0; u < CNT; ++u) { pv[u] = fl_ld<V>(g[u].p + e, true); xv[u] = fl_ld<V>(g[u].x + e, g[u].xa); }
#pragma unroll
    for (int u = 0; u < CNT; ++u) {
      const Pair x = {xv[u].a + co[u][c] * pv[u].a, V ? xv[u].b + co[u][V ? c + 1 : c] * pv[u].b : 0.0};
      fl_st<V>(g[u].x + e, x, g[u].xa, ((g[u].mask >> c) & 1u) != 0u, V && ((g[u].mask >> (c + 1)) & 1u) != 0u);
    }
    c += cstep; if (c >= k) c -= k;
  }
}

template <bool V>
__global__ __launch_bounds__(kRedThreads) void mscgn_update_kernel(size_t ne, int k, double *X, size_t ldx, const double *P, double *Ps,
                                                                  size_t ldp, const double *__restrict__ st, const double *__restrict__ ms,
                                                                  const double *__restrict__ sl)
{
  static_assert(kMscgGroup == 4, "the dispatch below is on 1..4");
  if (st[kStDone] != 0.0) return;
  __shared__ double co[kMscgGroup][kPcgnMaxRhs];
  const int nall = __builtin_amdgcn_readfirstlane((int)sl[kSlNBase] + (int)sl[kSlNLive]);
  for (int at = 0; at < nall; at += kMscgGroup) {
    const int cnt = nall - at < kMscgGroup ? nall - at : kMscgGroup;
    __syncthreads();                                         // the group before has read its table
    const int u = threadIdx.x / kPcgnMaxRhs, c = threadIdx.x % kPcgnMaxRhs;
    if (u < cnt && c < k) co[u][c] = ms[c * kMscgStateDoubles + (int)sl[kSlList + at + u] * kMsStride + kMsA];
    __syncthreads();
    if (cnt == 4)      mscgn_update_group<4, V>(ne, k, at, X, ldx, P, Ps, ldp, sl, co);
    else if (cnt == 3) mscgn_update_group<3, V>(ne, k, at, X, ldx, P, Ps, ldp, sl, co);
    else if (cnt == 2) mscgn_update_group<2, V>(ne, k, at, X, ldx, P, Ps, ldp, sl, co);
    else               mscgn_update_group<1, V>(ne, k, at, X, ldx, P, Ps, ldp, sl, co);
  }
}

// p_j = r_j + beta_j p_j for the live columns (FIRST: the first group rides in this pass), P_ij = z_ij r_j + b_ij P_ij for the live
// pairs of CNT shifts with sigma != 0 (z the new one): R is read once per group
template <int CNT, bool V, bool FIRST>
__device__ __forceinline__ void mscgn_direction_group(size_t ne, int k, int at, unsigned live, double *__restrict__ P,
                                                      const double *__restrict__ R, double *Ps, size_t ldp, const double *__restrict__ sl,
                                                      const double (&zc)[kMscgGroup][kPcgnMaxRhs], const double (&bc)[kMscgGroup][kPcgnMaxRhs],
                                                      const double (&be)[kPcgnMaxRhs])
{
  constexpr int W = V ? 2 : 1;
  MscgnShift g[CNT + 1];
#pragma unroll
  for (int u = 0; u < CNT; ++u) g[u] = mscgn_shift(sl, at + u, nullptr, 0, P, Ps, ldp);
  const size_t stride = (size_t)gridDim.x * kRedThreads * W;
  size_t e = ((size_t)blockIdx.x * kRedThreads + threadIdx.x) * W;
  int c = (int)(e % (size_t)k);
  const int cstep = (int)(stride % (size_t)k);
  for (; e < ne; e += stride) {
    const int c1 = V ? c + 1 : c;
    Pair pv[CNT + 1], p0 = {0.0, 0.0};
#pragma unroll
    for (int u = 0; u < CNT; ++u) pv[u] = fl_ld<V>(g[u].pw + e, true);
    const Pair r = fl_ld<V>(R + e, true);
    if (FIRST) {
      p0 = fl_ld<V>(P + e, true);
      const Pair p = {r.a + be[c] * p0.a, V ? r.b + be[c1] * p0.b : 0.0};
      fl_st<V>(P + e, p, true, ((live >> c) & 1u) != 0u, V && ((live >> c1) & 1u) != 0u);
    }
#pragma unroll
    for (int u = 0; u < CNT; ++u) {
      const double t1 = zc[u][c] * r.a, t2 = bc[u][c] * pv[u].a;
      const double t3 = V ? zc[u][c1] * r.b : 0.0, t4 = V ? bc[u][c1] * pv[u].b : 0.0;
      fl_st<V>(g[u].pw + e, {t1 + t2, t3 + t4}, true, ((g[u].mask >> c) & 1u) != 0u, V && ((g[u].mask >> c1) & 1u) != 0u);
    }
    c += cstep; if (c >= k) c -= k;
  }
}

template <int CNT, bool V, typename... T>
__device__ __forceinline__ void mscgn_direction_first(bool first, T &&...a)
{
  if (first) mscgn_direction_group<CNT, V, true>(a...);
  else mscgn_direction_group<CNT, V, false>(a...);
}

template <bool V>
__global__ __launch_bounds__(kRedThreads) void mscgn_direction_kernel(size_t ne, int k, double *__restrict__ P, const double *__restrict__ R,
                                                                     double *Ps, size_t ldp, const double *__restrict__ st,
                                                                     const double *__restrict__ cst, const double *__restrict__ ms,
                                                                     const double *__restrict__ sl)
{
  if (st[kStDone] != 0.0) return;
  __shared__ double zc[kMscgGroup][kPcgnMaxRhs], bc[kMscgGroup][kPcgnMaxRhs], be[kPcgnMaxRhs];
  const unsigned live = pcgn_live(st);
  const int nb = __builtin_amdgcn_readfirstlane((int)sl[kSlNBase]), nl = __builtin_amdgcn_readfirstlane((int)sl[kSlNLive]);
  if ((int)threadIdx.x < k) be[threadIdx.x] = cst[threadIdx.x * kStDoubles + kStBeta];
  for (int g0 = 0; g0 == 0 || g0 < nl; g0 += kMscgGroup) {
    const int cnt = nl - g0 < kMscgGroup ? nl - g0 : kMscgGroup, at = nb + g0;
    __syncthreads();                                         // the group before has read its tables
    const int u = threadIdx.x / kPcgnMaxRhs, c = threadIdx.x % kPcgnMaxRhs;
    if (u < cnt && c < k) {
      const double *e = ms + c * kMscgStateDoubles + (int)sl[kSlList + at + u] * kMsStride;
      zc[u][c] = e[kMsZ]; bc[u][c] = e[kMsB];
    }
    __syncthreads();
    if (cnt == 4)      mscgn_direction_first<4, V>(g0 == 0, ne, k, at, live, P, R, Ps, ldp, sl, zc, bc, be);
    else if (cnt == 3) mscgn_direction_first<3, V>(g0 == 0, ne, k, at, live, P, R, Ps, ldp, sl, zc, bc, be);
    else if (cnt == 2) mscgn_direction_first<2, V>(g0 == 0, ne, k, at, live, P, R, Ps, ldp, sl, zc, bc, be);
    else if (cnt == 1) mscgn_direction_first<1, V>(g0 == 0, ne, k, at, live, P, R, Ps, ldp, sl, zc, bc, be);
    else               mscgn_direction_group<0, V, true>(ne, k, at, live, P, R, Ps, ldp, sl, zc, bc, be);
  }
}

// the kernels' shape for k columns: KMAX = 4, 8, 16 or 32 sums per thread, VEC as in pcgn_init_kernel
template <int KMAX, int VEC> struct PcgnShape { static constexpr int kmax = KMAX, vec = VEC; };
template <int KMAX, typename F>
int pcgn_dispatch_vec(int vec, F f)
{
  return vec == 0 ? f(PcgnShape<KMAX, 0>{}) : vec == 1 ? f(PcgnShape<KMAX, 1>{}) : f(PcgnShape<KMAX, 2>{});
}

template <typename F>
int pcgn_dispatch(int k, int vec, F f)
{
  return k <= 4 ? pcgn_dispatch_vec<4>(vec, f) : k <= 8 ? pcgn_dispatch_vec<8>(vec, f) : k <= 16 ? pcgn_dispatch_vec<16>(vec, f)
                                                                                                   : pcgn_dispatch_vec<32>(vec, f);
}

struct Workspace {
  std::vector<void *> bufs;
  double *get(size_t n)
  {
    void *p = nullptr;
    if (hipMalloc(&p, sizeof(double) * (n ? n : 1)) != hipSuccess) return nullptr;
    bufs.push_back(p);
    return (double *)p;
  }
  ~Workspace() { for (void *p : bufs) (void)hipFree(p); }
};

// ---- the vector steps of fs_cg and fs_pcg as launchers, for callers that bring their own products (fs_dist_cg, fs_dist_pcg: the
// same steps on every rank of a row-sharded matrix -- same kernels on the same data, so every rank takes the same decisions).
// Every step that takes sums has ONE launcher and is told where they go (CgSums): whole-vector sums are finished by
// final_step_kernel, a slice's sums by final_sum_kernel into the rank's send slot -- and, gathered, by cg_dev_final.

// The one-workgroup kernel that finishes nv sums of `count` partials each and takes the scalar step: false where fs_cg and fs_pcg
// have no such step
static bool launch_final_step(CgStep step, int nv, const double *partials, int count, double *red, double *st, double arg, hipStream_t s)
{
  const dim3 one(1), blk(kRedThreads);
  switch ((int)step * 4 + nv) {
    case kStepCgStart * 4 + 1:  hipLaunchKernelGGL((final_step_kernel<1, kStepCgStart>), one, blk, 0, s, partials, count, red, st, arg); return true;
    case kStepCgAlpha * 4 + 1:  hipLaunchKernelGGL((final_step_kernel<1, kStepCgAlpha>), one, blk, 0, s, partials, count, red, st, arg); return true;
    case kStepCgBeta * 4 + 1:   hipLaunchKernelGGL((final_step_kernel<1, kStepCgBeta>), one, blk, 0, s, partials, count, red, st, arg); return true;
    case kStepPcgStart * 4 + 2: hipLaunchKernelGGL((final_step_kernel<2, kStepPcgStart>), one, blk, 0, s, partials, count, red, st, arg); return true;
    case kStepPcgRz * 4 + 1:    hipLaunchKernelGGL((final_step_kernel<1, kStepPcgRz>), one, blk, 0, s, partials, count, red, st, arg); return true;
    case kStepPcgBeta * 4 + 1:  hipLaunchKernelGGL((final_step_kernel<1, kStepPcgBeta>), one, blk, 0, s, partials, count, red, st, arg); return true;
    case kStepPcgBeta * 4 + 2:  hipLaunchKernelGGL((final_step_kernel<2, kStepPcgBeta>), one, blk, 0, s, partials, count, red, st, arg); return true;
    default: return false;
  }
}

// behind a vector kernel that left nv sums per workgroup in S.part
static int finish_sums(const CgSums &S, CgStep step, int nv, double arg, hipStream_t s)
{
  if (S.slice) {
    if (nv == 2) hipLaunchKernelGGL(final_sum_kernel<2>, dim3(1), dim3(kRedThreads), 0, s, S.part, kRedBlocks, S.slice);
    else         hipLaunchKernelGGL(final_sum_kernel<1>, dim3(1), dim3(kRedThreads), 0, s, S.part, kRedBlocks, S.slice);
  } else if (!launch_final_step(step, nv, S.part, kRedBlocks, S.red, S.st, arg, s)) {
    set_error("CG launcher: no scalar step for these sums"); return FS_ERR_ARG;
  }
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// fs_cg's start: x = 0, r = p = b; b.b, the stopping threshold
int cg_dev_init(int n, const double *b, double *x, double *r, double *p, const CgSums &S, double tol, hipStream_t s)
{
  hipLaunchKernelGGL(cg_init_kernel, dim3(kRedBlocks), dim3(kRedThreads), 0, s, n, b, x, r, p, S.part);
  return finish_sums(S, kStepCgStart, 1, tol, s);
}

// fs_pcg's.  cold: x = 0, r = b; warm (q = A'(A x) on entry): q += lambda x, r = b - q; then {b.b, r.r}, stop, done?
int pcg_dev_init(int n, bool warm, double lambda, const double *b, double *x, double *r, double *q, const CgSums &S, double tol,
                 hipStream_t s)
{
  if (warm) hipLaunchKernelGGL(pcg_init_kernel<true>, dim3(kRedBlocks), dim3(kRedThreads), 0, s, n, lambda, b, x, r, q, S.part);
  else      hipLaunchKernelGGL(pcg_init_kernel<false>, dim3(kRedBlocks), dim3(kRedThreads), 0, s, n, lambda, b, x, r, q, S.part);
  return finish_sums(S, kStepPcgStart, 2, tol, s);
}

// p = z = r dinv (dinv NULL: r), r.z
int pcg_dev_start(int n, const double *r, const double *dinv, double *p, const CgSums &S, hipStream_t s)
{
  if (dinv) hipLaunchKernelGGL(pcg_start_kernel<true>, dim3(kRedBlocks), dim3(kRedThreads), 0, s, n, r, dinv, p, S.part, S.st);
  else      hipLaunchKernelGGL(pcg_start_kernel<false>, dim3(kRedBlocks), dim3(kRedThreads), 0, s, n, r, dinv, p, S.part, S.st);
  return finish_sums(S, kStepPcgRz, 1, 0.0, s);
}

// behind q = A'(A p): q += lambda p, p.q; alpha = rsq_old / p.q (fs_pcg: r.z / p.q)
int cg_dev_shift_dot(int n, double lambda, const double *p, double *q, const CgSums &S, hipStream_t s)
{
  hipLaunchKernelGGL(cg_shift_dot_dev_kernel, dim3(kRedBlocks), dim3(kRedThreads), 0, s, n, lambda, q, p, S.part, S.st);
  return finish_sums(S, kStepCgAlpha, 1, 0.0, s);
}

// x and r; r.r, or {r.r, r.z} with a preconditioner; `beta` is the convergence step: kStepCgBeta, or fs_pcg's kStepPcgBeta (it
// also keeps r.r)
int cg_dev_update(int n, double *x, double *r, const double *p, const double *q, const double *dinv, const CgSums &S, CgStep beta,
                  hipStream_t s)
{
  if (dinv) hipLaunchKernelGGL(pcg_update_kernel, dim3(kRedBlocks), dim3(kRedThreads), 0, s, n, x, r, p, q, dinv, S.part, S.st);
  else      hipLaunchKernelGGL(cg_update_dev_kernel, dim3(kRedBlocks), dim3(kRedThreads), 0, s, n, x, r, p, q, S.part, S.st);
  return finish_sums(S, beta, dinv ? 2 : 1, 0.0, s);
}

// the new p = z + beta p
int cg_dev_direction(int n, double *p, const double *r, const double *dinv, const double *st, hipStream_t s)
{
  if (dinv) hipLaunchKernelGGL(pcg_direction_kernel, dim3(kRedBlocks), dim3(kRedThreads), 0, s, n, p, r, dinv, st);
  else      hipLaunchKernelGGL(cg_direction_dev_kernel, dim3(kRedBlocks), dim3(kRedThreads), 0, s, n, p, r, st);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// everything of an iteration behind q = A'(A p) on whole vectors, all on the device.  fs_cg: (NULL, kStepCgBeta); fs_pcg:
// kStepPcgBeta -- without a preconditioner it runs fs_cg's launches with its own convergence step
int cg_dev_steps(int n, double lambda, double *x, double *r, double *p, double *q, const double *dinv, const CgSums &S, CgStep beta,
                 hipStream_t s)
{
  if (int rc = cg_dev_shift_dot(n, lambda, p, q, S, s)) return rc;
  if (int rc = cg_dev_update(n, x, r, p, q, dinv, S, beta, s)) return rc;
  return cg_dev_direction(n, p, r, dinv, S.st, s);
}

// the sums of every rank's slice, gathered.  `partials`: count x nv doubles, rank-major as the exchange leaves them --
// block_sum<NV>'s own layout, so every one of the nv sums is finish_sum's tree (stage 2) over its count values.  nv = 2 for
// kStepPcgStart {b.b, r.r} and for kStepPcgBeta with a preconditioner {r.r, r.z}; red_out has room for nv doubles
int cg_dev_final(CgStep step, const double *partials, int count, double *red_out, double *st, double arg, hipStream_t s, int nv)
{
  const bool pcg2 = (step == kStepPcgStart) || (step == kStepPcgBeta && nv == 2);
  if (nv != (pcg2 ? 2 : 1)) { set_error("cg_dev_final: the step does not take this many sums"); return FS_ERR_ARG; }
  if (!launch_final_step(step, nv, partials, count, red_out, st, arg, s)) {
    set_error("cg_dev_final: not a step of fs_cg or fs_pcg"); return FS_ERR_ARG;
  }
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// dinv = 1 / d, 1 where d is 0; in place or not
int pcg_dev_dinv(int n, const double *d, double *dinv, hipStream_t s)
{
  hipLaunchKernelGGL(pcg_dinv_kernel, dim3(kRedBlocks), dim3(kRedThreads), 0, s, n, d, dinv);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// what fs_pcg, fs_pcgn and their sharded forms refuse in a fs_pcg_params, in this order, in `who`'s name
int pcg_params_ok(const char *who, const fs_pcg_params *prm)
{
  const std::string w(who);
  if (prm->precond != FS_PRECOND_NONE && prm->precond != FS_PRECOND_JACOBI && prm->precond != FS_PRECOND_DIAG) {
    set_error(w + ": precond is none of FS_PRECOND_NONE / _JACOBI / _DIAG"); return FS_ERR_ARG;
  }
  if (prm->precond == FS_PRECOND_DIAG && !prm->diag) { set_error(w + ": FS_PRECOND_DIAG without a diagonal"); return FS_ERR_ARG; }
  if (!(prm->tol >= 0.0)) { set_error(w + ": tol is negative or NaN"); return FS_ERR_ARG; }
  return FS_OK;
}

// fs_pcg_info from the final st[] of a solve
void pcg_info_of(const double *fin, fs_pcg_info *info)
{
  if (!info) return;
  info->iterations = (int)fin[kStIter];
  info->converged = fin[kStDone] != 0.0;
  info->rnorm = sqrt(fin[kStRr]);
  info->bnorm = sqrt(fin[kStBb]);
}

// ---- fs_pcgn's steps as launchers (fs_pcgn, fs_pcgn_lambdas; fs_dist_pcgn and fs_dist_pcgn_lambdas on every rank, on whole panels
// or on the rank's slice).  part: pcgn_part_doubles(k), cs: kPcgnStateDoubles.
// 16-byte accesses: R, P, Q are the solve's own (rows of an even k stay aligned, and a slice starts at its own allocation), X and B
// may be the caller's
static int pcgn_vec(int k, const double *X, const double *B)
{
  return (k & 1) ? 0 : ((((uintptr_t)X | (uintptr_t)B) & 15) == 0 ? 2 : 1);
}

int pcgn_dev_clear(double *cs, hipStream_t s)     // slots a column never writes read as 0 in the debug getter
{
  FS_HIP(hipMemsetAsync(cs, 0, sizeof(double) * kPcgnMaxRhs * kPnStride, s));
  return FS_OK;
}

// One launcher per step, for whole panels and for a rank's slice alike (n rows on the slice's pointers).  LAM: the solve's one
// lambda (double: fs_pcgn's instantiations) or its k (PcgnLambdas: fs_pcgn_lambdas).  colj: nothing, or the k lambdas again when
// dinv holds s = diag(A'A) and the kernels invert s + lambda_c per element; without it the kernels behind the first one see no
// lambda and are fs_pcgn's own.  vec: pcgn_vec of the solve's X and B.  Behind a step that takes sums, pcgn_sums_launch.

// the scalar step behind ns sums per column: over the kRedBlocks partials of whole panels, or (RANKS) over `count` ranks' values
template <bool RANKS>
static void pcgn_step_launch(PcgnStep step, const double *part, int count, double *st, double *cs, int k, int ns, double tol, hipStream_t s)
{
  const dim3 one(1), blk(kRedThreads);
  switch (step) {
    case kPnStepStart: hipLaunchKernelGGL((pcgn_step_kernel<kPnStepStart, RANKS>), one, blk, 0, s, part, count, st, cs, k, ns, tol); break;
    case kPnStepRz:    hipLaunchKernelGGL((pcgn_step_kernel<kPnStepRz, RANKS>), one, blk, 0, s, part, count, st, cs, k, ns, tol); break;
    case kPnStepAlpha: hipLaunchKernelGGL((pcgn_step_kernel<kPnStepAlpha, RANKS>), one, blk, 0, s, part, count, st, cs, k, ns, tol); break;
    default:           hipLaunchKernelGGL((pcgn_step_kernel<kPnStepBeta, RANKS>), one, blk, 0, s, part, count, st, cs, k, ns, tol); break;
  }
}

// ns finished sums per column into `send`: of the kRedBlocks partials in `part` (ranks = 0), or of `ranks` ranks' gathered slots
static void pcgn_fold_launch(const double *part, int ranks, double *send, const double *st, int k, int ns, bool start, hipStream_t s)
{
  hipLaunchKernelGGL(pcgn_fold_kernel, dim3(1), dim3(kRedThreads), 0, s, part, ranks, send, st, k, ns, (int)start);
}

// behind a vector kernel that left ns sums per live column and workgroup in U.part: whole panels are finished and the scalar
// step taken; a slice's sums are folded into the rank's send slot
static void pcgn_sums_launch(PcgnStep step, const PcgnSums &U, int k, int ns, double tol, hipStream_t s)
{
  if (U.send) pcgn_fold_launch(U.part, 0, U.send, U.st, k, ns, step == kPnStepStart, s);
  else pcgn_step_launch<false>(step, U.part, kRedBlocks, U.st, U.cs, k, ns, tol, s);
}

// cold: X = 0, R = B; warm (Q = A'(A X) on entry): Q += lambda X, R = B - Q; b.b, r.r, stop, live? per column
template <typename LAM>
static int pcgn_init_step(int n, int k, int vec, bool warm, const LAM &lambda, const double *B, double *X, double *R, double *Q,
                          const PcgnSums &U, double tol, hipStream_t s)
{
  const int rc = pcgn_dispatch(k, vec, [&](auto sh) -> int {
    using S = decltype(sh);
    hipLaunchKernelGGL((pcgn_init_kernel<S::kmax, S::vec, LAM>), dim3(kRedBlocks), dim3(kRedThreads), 0, s, n, k, (int)warm, lambda, B, X, R, Q, U.part);
    return FS_OK;
  });
  pcgn_sums_launch(kPnStepStart, U, k, 2, tol, s);                                                           // b.b, r.r, stop, live?
  return rc;
}

// P = Z = R dinv, r.z
template <typename... CJ>
static int pcgn_start_step(int n, int k, int vec, const double *R, const double *dinv, double *P, const PcgnSums &U, hipStream_t s, CJ... colj)
{
  const int rc = pcgn_dispatch(k, vec, [&](auto sh) -> int {
    using S = decltype(sh);
    hipLaunchKernelGGL((pcgn_start_kernel<S::kmax, S::vec, CJ...>), dim3(kRedBlocks), dim3(kRedThreads), 0, s, n, k, R, dinv, P, U.part, U.st, colj...);
    return FS_OK;
  });
  pcgn_sums_launch(kPnStepRz, U, k, 1, 0.0, s);                                                              // r.z
  return rc;
}

// a per-iteration vector kernel in the form that option "pcgn_kernel" picks: the two forms of a step take the same arguments
template <typename K, typename... A>
static int pcgn_form_launch(int k, K *staged, K *rows, hipStream_t s, A... a)
{
  const int which = options().pcgn_kernel;
  K *const kernel = which == 2 || (which == 0 && k > kPcgnRowsMaxK) ? staged : rows;
  hipLaunchKernelGGL(kernel, dim3(kRedBlocks), dim3(kRedThreads), 0, s, a...);
  return FS_OK;
}

// behind Q = A'(A P): Q += lambda P, q.p; alpha = r.z / p.q
template <typename LAM>
static int pcgn_shift_dot_step(int n, int k, int vec, const LAM &lambda, double *Q, const double *P, const PcgnSums &U, hipStream_t s)
{
  const int rc = pcgn_dispatch(k, vec, [&](auto sh) -> int {
    using S = decltype(sh);
    return pcgn_form_launch(k, pcgn_shift_dot_lds_kernel<S::kmax, LAM>, pcgn_shift_dot_kernel<S::kmax, S::vec, LAM>, s,
                            n, k, lambda, Q, P, U.part, U.st);
  });
  pcgn_sums_launch(kPnStepAlpha, U, k, 1, 0.0, s);                                                           // alpha = r.z / p.q
  return rc;
}

// X (NULL: left to the caller's own steps) and R; r.r, or {r.r, r.z} with a preconditioner: converged? beta
template <typename... CJ>
static int pcgn_update_step(int n, int k, int vec, double *X, double *R, const double *P, const double *Q, const double *dinv,
                            const PcgnSums &U, hipStream_t s, CJ... colj)
{
  const int rc = pcgn_dispatch(k, vec, [&](auto sh) -> int {
    using S = decltype(sh);
    auto launch = [&](auto xup) {
      constexpr bool XUP = decltype(xup)::value;
      return pcgn_form_launch(k, pcgn_update_lds_kernel<S::kmax, XUP, CJ...>, pcgn_update_kernel<S::kmax, S::vec, XUP, CJ...>, s,
                              n, k, X, R, P, Q, dinv, U.part, U.st, U.cs, colj...);
    };
    if constexpr (sizeof...(CJ) == 0) {
      if (!X) return launch(std::false_type{});                          // X NULL (fs_mscgn): r and its sums only
    }
    return launch(std::true_type{});
  });
  pcgn_sums_launch(kPnStepBeta, U, k, dinv ? 2 : 1, 0.0, s);                                                 // converged? beta
  return rc;
}

// the new P = Z + beta P
template <typename... CJ>
static int pcgn_direction_step(int n, int k, int vec, double *P, const double *R, const double *dinv, const PcgnSums &U, hipStream_t s,
                               CJ... colj)
{
  const int rc = pcgn_dispatch(k, vec, [&](auto sh) -> int {
    using S = decltype(sh);
    return pcgn_form_launch(k, pcgn_direction_lds_kernel<S::kmax, CJ...>, pcgn_direction_kernel<S::kmax, S::vec, CJ...>, s,
                            n, k, P, R, dinv, U.st, U.cs, colj...);
  });
  FS_HIP(hipGetLastError());
  return rc;
}

// the start of a solve on whole panels: the two steps in sequence, each with its scalar step behind it
template <typename LAM, typename... CJ>
static int pcgn_init_launch(int n, int k, bool warm, const LAM &lambda, const double *B, double *X, double *R, double *P, double *Q,
                            const double *dinv, double *part, double *st, double *cs, double tol, hipStream_t s, CJ... colj)
{
  const PcgnSums U{part, st, cs, nullptr};
  const int vec = pcgn_vec(k, X, B);
  if (int rc = pcgn_init_step(n, k, vec, warm, lambda, B, X, R, Q, U, tol, s)) return rc;
  if (int rc = pcgn_start_step(n, k, vec, R, dinv, P, U, s, colj...)) return rc;
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// everything of an iteration behind Q = A'(A P) on whole panels.  LAM, colj: as above
template <typename LAM, typename... CJ>
static int pcgn_steps_launch(int n, int k, const LAM &lambda, double *X, const double *B, double *R, double *P, double *Q,
                             const double *dinv, double *part, double *st, double *cs, hipStream_t s, CJ... colj)
{
  const PcgnSums U{part, st, cs, nullptr};
  const int vec = pcgn_vec(k, X, B);
  if (int rc = pcgn_shift_dot_step(n, k, vec, lambda, Q, P, U, s)) return rc;
  if (int rc = pcgn_update_step(n, k, vec, X, R, P, Q, dinv, U, s, colj...)) return rc;
  return pcgn_direction_step(n, k, vec, P, R, dinv, U, s, colj...);
}

int pcgn_dev_init(int n, int k, bool warm, double lambda, const double *B, double *X, double *R, double *P, double *Q, const double *dinv,
                  double *part, double *st, double *cs, double tol, hipStream_t s)
{
  return pcgn_init_launch(n, k, warm, lambda, B, X, R, P, Q, dinv, part, st, cs, tol, s);
}

int pcgn_dev_steps(int n, int k, double lambda, double *X, const double *B, double *R, double *P, double *Q, const double *dinv,
                   double *part, double *st, double *cs, hipStream_t s)
{
  return pcgn_steps_launch(n, k, lambda, X, B, R, P, Q, dinv, part, st, cs, s);
}

// fs_pcgn_lambdas' instantiations on whole panels (fs_pcgn_lambdas; fs_dist_pcgn_lambdas replicated, on every rank).  colj: dinv
// holds s = diag(A'A) at 0.0 and every column inverts s + lambda_c (FS_PRECOND_JACOBI): f takes the k lambdas again as its
// trailing argument, or none
template <typename F>
static int pcgn_with_colj(bool colj, const PcgnLambdas &lv, F f)
{
  return colj ? f(lv) : f();
}

int pcgn_dev_init_lambdas(int n, int k, bool warm, const PcgnLambdas &lv, bool colj, const double *B, double *X, double *R, double *P,
                          double *Q, const double *dinv, double *part, double *st, double *cs, double tol, hipStream_t s)
{
  return pcgn_with_colj(colj, lv, [&](auto... cj) { return pcgn_init_launch(n, k, warm, lv, B, X, R, P, Q, dinv, part, st, cs, tol, s, cj...); });
}

int pcgn_dev_steps_lambdas(int n, int k, const PcgnLambdas &lv, bool colj, double *X, const double *B, double *R, double *P, double *Q,
                           const double *dinv, double *part, double *st, double *cs, hipStream_t s)
{
  return pcgn_with_colj(colj, lv, [&](auto... cj) { return pcgn_steps_launch(n, k, lv, X, B, R, P, Q, dinv, part, st, cs, s, cj...); });
}

// the same steps one by one on a rank's slice of n rows (fs_dist_pcgn_lambdas on slices): U.send is the rank's send slot, the
// exchange and pcgn_dev_rank_step follow each step that takes sums.  X, B, R, Q: the slice; P: the slice of the direction
int pcgn_slice_init(int n, int k, bool warm, const PcgnLambdas &lv, const double *B, double *X, double *R, double *Q, const PcgnSums &U,
                    hipStream_t s)
{
  if (int rc = pcgn_init_step(n, k, pcgn_vec(k, X, B), warm, lv, B, X, R, Q, U, 0.0, s)) return rc;
  FS_HIP(hipGetLastError());
  return FS_OK;
}

int pcgn_slice_start(int n, int k, const PcgnLambdas &lv, bool colj, const double *X, const double *B, const double *R, const double *dinv,
                     double *P, const PcgnSums &U, hipStream_t s)
{
  if (int rc = pcgn_with_colj(colj, lv, [&](auto... cj) { return pcgn_start_step(n, k, pcgn_vec(k, X, B), R, dinv, P, U, s, cj...); })) return rc;
  FS_HIP(hipGetLastError());
  return FS_OK;
}

int pcgn_slice_shift_dot(int n, int k, const PcgnLambdas &lv, const double *X, const double *B, double *Q, const double *P,
                         const PcgnSums &U, hipStream_t s)
{
  if (int rc = pcgn_shift_dot_step(n, k, pcgn_vec(k, X, B), lv, Q, P, U, s)) return rc;
  FS_HIP(hipGetLastError());
  return FS_OK;
}

int pcgn_slice_update(int n, int k, const PcgnLambdas &lv, bool colj, double *X, const double *B, double *R, const double *P,
                      const double *Q, const double *dinv, const PcgnSums &U, hipStream_t s)
{
  if (int rc = pcgn_with_colj(colj, lv, [&](auto... cj) { return pcgn_update_step(n, k, pcgn_vec(k, X, B), X, R, P, Q, dinv, U, s, cj...); }))
    return rc;
  FS_HIP(hipGetLastError());
  return FS_OK;
}

int pcgn_slice_direction(int n, int k, const PcgnLambdas &lv, bool colj, const double *X, const double *B, double *P, const double *R,
                         const double *dinv, const PcgnSums &U, hipStream_t s)
{
  return pcgn_with_colj(colj, lv, [&](auto... cj) { return pcgn_direction_step(n, k, pcgn_vec(k, X, B), P, R, dinv, U, s, cj...); });
}

// the slice sums of every rank, gathered (`all`: rank r's ns * k values at r * ns * k): stage 2 over the ranks in rank order per
// sum, then the scalar step.  ns: 2 for kPnStepStart {b.b, r.r} and for kPnStepBeta with a preconditioner {r.r, r.z}, else 1
int pcgn_dev_rank_step(PcgnStep step, const double *all, int nranks, int k, int ns, double tol, double *st, double *cs, hipStream_t s)
{
  pcgn_step_launch<true>(step, all, nranks, st, cs, k, ns, tol, s);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// option "pcgn_compact": up to three n x ws panels into n x wd panels by `map` (pcgn_repack_kernel; a NULL source is skipped)
static int pcgn_repack_launch(bool keep, int n, int ws, int wd, const PcgnColMap &map, const double *S0, const double *S1, const double *S2,
                              double *D0, double *D1, double *D2, const double *st, hipStream_t s)
{
  unsigned tiles = 0u;
  for (int c = 0; c < wd; ++c)
    if (map.v[c] >= 0) tiles |= 1u << (map.v[c] >> 4);
  const dim3 g(kRedBlocks), blk(kRedThreads);
  auto go = [&](auto kmax) {
    constexpr int KMAX = decltype(kmax)::value;
    if (keep) hipLaunchKernelGGL((pcgn_repack_kernel<KMAX, true>), g, blk, 0, s, n, ws, wd, map, tiles, S0, S1, S2, D0, D1, D2, st);
    else      hipLaunchKernelGGL((pcgn_repack_kernel<KMAX, false>), g, blk, 0, s, n, ws, wd, map, tiles, S0, S1, S2, D0, D1, D2, st);
  };
  if (ws <= 4) go(std::integral_constant<int, 4>{});
  else if (ws <= 8) go(std::integral_constant<int, 8>{});
  else if (ws <= 16) go(std::integral_constant<int, 16>{});
  else go(std::integral_constant<int, 32>{});
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// ---- fs_mscg's steps as launchers (fs_mscg; fs_dist_mscg on every rank: whole vectors, or the rank's slice of r, p, q, the x_i
// and the P_i).  The vector kernels take (n, part), the scalar kernels (partials, count): kRedBlocks partials of whole vectors, or
// the ranks' values, gathered.  A slice's sums go through final_sum_kernel into the send slot, as in finish_sums.

// what fs_mscg and fs_dist_mscg refuse in their arguments, in this order, in `who`'s name
int mscg_args_ok(const char *who, int F, int64_t ldx, int m, const double *lambda, double tol)
{
  const std::string w(who);
  if (m < 1 || m > kMscgMaxShifts) { set_error(w + ": m outside 1..FS_MSCG_MAX_SHIFTS"); return FS_ERR_ARG; }
  if (ldx < F) { set_error(w + ": ldx < ncol(A)"); return FS_ERR_ARG; }
  if (!(tol >= 0.0)) { set_error(w + ": tol is negative or NaN"); return FS_ERR_ARG; }
  for (int i = 0; i < m; ++i)
    if (!isfinite(lambda[i])) { set_error(w + ": a lambda is NaN or infinite"); return FS_ERR_ARG; }
  return FS_OK;
}

// the host's part of a solve: the base system, every shift's sigma and the number of direction vectors
MscgShifts mscg_shifts(int m, const double *lambda)
{
  double base = lambda[0];
  for (int i = 1; i < m; ++i) if (lambda[i] < base) base = lambda[i];
  MscgSigma sg;
  int nslots = 0;
  for (int i = 0; i < kMscgMaxShifts; ++i) {
    sg.v[i] = i < m ? lambda[i] - base : 0.0;                 // exactly 0 for the minimum and its duplicates
    if (sg.v[i] != 0.0) ++nslots;
  }
  return MscgShifts{base, sg, nslots};
}

// the one-workgroup kernel that finishes a sum of `count` partials and takes the scalar step
static int mscg_scalar_step(MscgStep step, const double *partials, int count, double *red, double *st, const MscgScalars &K, hipStream_t s)
{
  const dim3 one(1), blk(kRedThreads);
  if (step == kMscgStart)   hipLaunchKernelGGL(mscg_start_kernel, one, blk, 0, s, partials, count, red, st, K.ms, K.tol, K.m, K.sh->sg);
  else if (step == kMscgS1) hipLaunchKernelGGL(mscg_s1_kernel, one, blk, 0, s, partials, count, red, st, K.ms, K.m);   // alpha, the a_i
  else                      hipLaunchKernelGGL(mscg_s2_kernel, one, blk, 0, s, partials, count, red, st, K.ms, K.m);   // converged? beta, freezes
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// behind a vector kernel that left one sum per workgroup in S.part
static int mscg_finish_sums(const CgSums &S, MscgStep step, const MscgScalars &K, hipStream_t s)
{
  if (!S.slice) return mscg_scalar_step(step, S.part, kRedBlocks, S.red, S.st, K, s);
  hipLaunchKernelGGL(final_sum_kernel<1>, dim3(1), dim3(kRedThreads), 0, s, S.part, kRedBlocks, S.slice);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// x_i = 0 for the K.m shifts, r = p = b, P_i = b for the shifts with sigma != 0; b.b, stop, every shift's scalars, done?
int mscg_dev_init(int n, const double *b, double *r, double *p, double *X, long long ldx, double *P, long long ldp, const CgSums &S,
                  const MscgScalars &K, hipStream_t s)
{
  hipLaunchKernelGGL(mscg_init_kernel, dim3(kRedBlocks), dim3(kRedThreads), 0, s, n, b, r, p, X, ldx, K.m, P, ldp, K.sh->nslots, S.part);
  return mscg_finish_sums(S, kMscgStart, K, s);
}

// behind q = A'(A p): q += base p, q.p on fs_cg's kernel; S1
int mscg_dev_shift_dot(int F, double base, const double *p, double *q, const CgSums &S, const MscgScalars &K, hipStream_t s)
{
  const dim3 g(kRedBlocks), blk(kRedThreads);
  double *part = S.part;
  const double *st = S.st;
  hipLaunchKernelGGL(cg_shift_dot_dev_kernel, g, blk, 0, s, F, base, q, p, part, st);
  return mscg_finish_sums(S, kMscgS1, K, s);
}

// r and the x_i of the live shifts; r.r; S2
int mscg_dev_update(int n, double *r, const double *p, const double *q, double *X, long long ldx, const double *P, long long ldp,
                    const CgSums &S, const MscgScalars &K, hipStream_t s)
{
  hipLaunchKernelGGL(mscg_update_kernel, dim3(kRedBlocks), dim3(kRedThreads), 0, s, n, r, p, q, X, ldx, P, ldp, S.part, S.st, K.ms);
  return mscg_finish_sums(S, kMscgS2, K, s);
}

// the new p and the new P_i of the live shifts
int mscg_dev_direction(int n, double *p, const double *r, double *P, long long ldp, const double *st, const double *ms, hipStream_t s)
{
  hipLaunchKernelGGL(mscg_direction_kernel, dim3(kRedBlocks), dim3(kRedThreads), 0, s, n, p, r, P, ldp, st, ms);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// everything of an iteration behind q = A'(A p) on whole vectors, all on the device
int mscg_dev_steps(int n, double base, double *r, double *p, double *q, double *X, long long ldx, double *P, long long ldp, const CgSums &S,
                   const MscgScalars &K, hipStream_t s)
{
  if (int rc = mscg_dev_shift_dot(n, base, p, q, S, K, s)) return rc;
  if (int rc = mscg_dev_update(n, r, p, q, X, ldx, P, ldp, S, K, s)) return rc;
  return mscg_dev_direction(n, p, r, P, ldp, S.st, K.ms, s);
}

// the sums of every rank's slice, gathered: `partials` holds one value per rank, finish_sum's tree (stage 2) adds them in rank order
int mscg_dev_final(MscgStep step, const double *partials, int count, double *red_out, double *st, const MscgScalars &K, hipStream_t s)
{
  return mscg_scalar_step(step, partials, count, red_out, st, K, s);
}

// ---- fs_mscgn's steps as launchers (fs_mscgn; fs_dist_mscgn on every rank: whole panels, or the rank's slice of R, Q, the X_i and
// the P_i -- a slice starts on a row boundary, so it is a panel of fewer rows and the flat kernels take it as one).  fs_pcgn's
// launchers serve every step that takes per-column sums: pcgn_fold_kernel leaves them finished in U.send.  U.send == K.red: whole
// panels, the scalar step of fs_mscg per column (mscgn_step_kernel, which reads K.red) follows at once.  Else U.send is the rank's
// send slot, and the step comes with mscgn_dev_rank_step once the slots of all ranks are gathered.  The flat kernels do the pairs.
// F rows (a slice: its own), ne = F k elements per panel; Ps: the direction panels of the shifts with sigma != 0, ldp doubles apart
static int mscgn_scalar_step(MscgStep step, const PcgnSums &U, const MscgnScalars &K, int k, hipStream_t s)
{
  const dim3 one(1), blk(kRedThreads);
  if (step == kMscgStart)   hipLaunchKernelGGL(mscgn_step_kernel<kMscgStart>, one, blk, 0, s, K.red, U.st, K.cst, U.cs, K.ms, K.sl, k, K.m, K.tol, K.sh->sg);
  else if (step == kMscgS1) hipLaunchKernelGGL(mscgn_step_kernel<kMscgS1>, one, blk, 0, s, K.red, U.st, K.cst, U.cs, K.ms, K.sl, k, K.m, K.tol, K.sh->sg);
  else                      hipLaunchKernelGGL(mscgn_step_kernel<kMscgS2>, one, blk, 0, s, K.red, U.st, K.cst, U.cs, K.ms, K.sl, k, K.m, K.tol, K.sh->sg);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// behind a step whose finished sums pcgn_fold_kernel left in U.send
static int mscgn_finish_sums(MscgStep step, const PcgnSums &U, const MscgnScalars &K, int k, hipStream_t s)
{
  if (U.send == K.red) return mscgn_scalar_step(step, U, K, k, s);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// X_i = 0 for the K.m shifts, R = P = B, P_i = B for the shifts with sigma != 0; {b.b, r.r} per column: start
int mscgn_dev_init(int F, int k, const double *B, double *X, long long ldx, double *R, double *P, double *Q, double *Ps, long long ldp,
                   const PcgnSums &U, const MscgnScalars &K, hipStream_t s)
{
  if (int rc = pcgn_init_step(F, k, pcgn_vec(k, X, B), false, 0.0, B, X, R, Q, U, K.tol, s)) return rc;   // X_0 = 0, R = B; {b.b, r.r}
  if (int rc = mscgn_finish_sums(kMscgStart, U, K, k, s)) return rc;
  const size_t ne = (size_t)F * k;
  const dim3 g(kRedBlocks), blk(kRedThreads);
  if (k & 1) hipLaunchKernelGGL(mscgn_fill_kernel<false>, g, blk, 0, s, ne, B, P, Ps, (size_t)ldp, K.sh->nslots, X, (size_t)ldx, K.m);
  else       hipLaunchKernelGGL(mscgn_fill_kernel<true>, g, blk, 0, s, ne, B, P, Ps, (size_t)ldp, K.sh->nslots, X, (size_t)ldx, K.m);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// behind Q = A'(A P): Q += base P, q.p per live column: S1 (alpha_j, the a_ij).  R, P, Q are the solve's own: 16-byte forms for even k
int mscgn_dev_shift_dot(int F, int k, double *Q, const double *P, const PcgnSums &U, const MscgnScalars &K, hipStream_t s)
{
  const int vec = (k & 1) ? 0 : 1;
  if (int rc = pcgn_shift_dot_step(F, k, vec, K.sh->base, Q, P, U, s)) return rc;
  return mscgn_finish_sums(kMscgS1, U, K, k, s);
}

// R -= alpha Q with r.r per live column, then x_ij += a_ij P_ij for the live pairs: S2 (converged?  beta_j, freezes)
int mscgn_dev_update(int F, int k, double *X, long long ldx, double *R, const double *P, const double *Q, double *Ps, long long ldp,
                     const PcgnSums &U, const MscgnScalars &K, hipStream_t s)
{
  const size_t ne = (size_t)F * k;
  const dim3 g(kRedBlocks), blk(kRedThreads);
  const int vec = (k & 1) ? 0 : 1;
  if (int rc = pcgn_update_step(F, k, vec, nullptr, R, P, Q, nullptr, U, s)) return rc;
  if (k & 1) hipLaunchKernelGGL(mscgn_update_kernel<false>, g, blk, 0, s, ne, k, X, (size_t)ldx, P, Ps, (size_t)ldp, U.st, K.ms, K.sl);
  else       hipLaunchKernelGGL(mscgn_update_kernel<true>, g, blk, 0, s, ne, k, X, (size_t)ldx, P, Ps, (size_t)ldp, U.st, K.ms, K.sl);
  return mscgn_finish_sums(kMscgS2, U, K, k, s);
}

// the new P and the new P_ij of the live pairs
int mscgn_dev_direction(int F, int k, double *P, const double *R, double *Ps, long long ldp, const PcgnSums &U, const MscgnScalars &K,
                        hipStream_t s)
{
  const size_t ne = (size_t)F * k;
  const dim3 g(kRedBlocks), blk(kRedThreads);
  if (k & 1) hipLaunchKernelGGL(mscgn_direction_kernel<false>, g, blk, 0, s, ne, k, P, R, Ps, (size_t)ldp, U.st, K.cst, K.ms, K.sl);
  else       hipLaunchKernelGGL(mscgn_direction_kernel<true>, g, blk, 0, s, ne, k, P, R, Ps, (size_t)ldp, U.st, K.cst, K.ms, K.sl);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// everything of an iteration behind Q = A'(A P) on whole panels, all on the device
int mscgn_dev_steps(int F, int k, double *X, long long ldx, double *R, double *P, double *Q, double *Ps, long long ldp, const PcgnSums &U,
                    const MscgnScalars &K, hipStream_t s)
{
  if (int rc = mscgn_dev_shift_dot(F, k, Q, P, U, K, s)) return rc;
  if (int rc = mscgn_dev_update(F, k, X, ldx, R, P, Q, Ps, ldp, U, K, s)) return rc;
  return mscgn_dev_direction(F, k, P, R, Ps, ldp, U, K, s);
}

// the send slots of every rank, gathered (`all`: rank r's ns * k values at r * ns * k; ns = 2 for the start, else 1): each sum
// over the ranks in rank order into K.red -- pcgn_step_kernel<STEP, true>'s fold -- then the scalar step, on every rank over the
// same values
int mscgn_dev_rank_step(MscgStep step, const double *all, int nranks, int k, const PcgnSums &U, const MscgnScalars &K, hipStream_t s)
{
  pcgn_fold_launch(all, nranks, K.red, U.st, k, step == kMscgStart ? 2 : 1, step == kMscgStart, s);
  return mscgn_scalar_step(step, U, K, k, s);
}

// ---- the same for two right-hand sides (fs_cg2, fs_dist_cg2).  cg2_dev_init is synchronous (two reductions go to the host: the
// norms of B's columns scale the system, cg.h:105-125); norms[2] is returned for the final cg2_dev_finish
int cg2_dev_init(int n, const double *B, double *X, double *R, double *P, double *part, double *red, double *st, double tol,
                 double *norms, hipStream_t s)
{
  const dim3 g(kRedBlocks), blk(kRedThreads);
  double h[3], RtR[3];
  hipLaunchKernelGGL(cg2_dot_kernel, g, blk, 0, s, n, B, B, part);
  hipLaunchKernelGGL(final_sum_kernel<3>, dim3(1), blk, 0, s, part, kRedBlocks, red);
  FS_HIP(hipGetLastError());
  FS_HIP(hipMemcpyAsync(h, red, sizeof(h), hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  norms[0] = sqrt(h[0]); norms[1] = sqrt(h[1]);
  hipLaunchKernelGGL(cg2_init_kernel, g, blk, 0, s, n, 1.0 / norms[0], 1.0 / norms[1], B, X, R, P, part);
  hipLaunchKernelGGL(final_sum_kernel<3>, dim3(1), blk, 0, s, part, kRedBlocks, red);
  FS_HIP(hipGetLastError());
  FS_HIP(hipMemcpyAsync(RtR, red, sizeof(RtR), hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  double st0[kStDoubles] = {0.0};
  st0[kSt2RtR] = RtR[0]; st0[kSt2RtR + 1] = RtR[1]; st0[kSt2RtR + 2] = RtR[2]; st0[kSt2Tolsq] = tol * tol;
  FS_HIP(hipMemcpyAsync(st, st0, sizeof(st0), hipMemcpyHostToDevice, s));
  FS_HIP(hipStreamSynchronize(s));            // (st0 is on this stack frame)
  return FS_OK;
}

// everything of a block-CG iteration behind Q = A'(A P): Q += lambda P, Alpha, X and R, the convergence test and Psi, the new P
int cg2_dev_steps(int n, double lambda, double *X, double *R, double *P, double *Q, double *part, double *red, double *st, hipStream_t s)
{
  const dim3 g(kRedBlocks), blk(kRedThreads), one(1);
  hipLaunchKernelGGL(cg2_shift_dot_dev_kernel, g, blk, 0, s, n, lambda, Q, P, part, st);
  hipLaunchKernelGGL((final_step_kernel<3, kStepCg2Alpha>), one, blk, 0, s, part, kRedBlocks, red, st, 0.0);   // Alpha
  hipLaunchKernelGGL(cg2_update_dev_kernel, g, blk, 0, s, n, X, R, P, Q, part, st);
  hipLaunchKernelGGL((final_step_kernel<3, kStepCg2Psi>), one, blk, 0, s, part, kRedBlocks, red, st, 0.0);   // converged? Psi
  hipLaunchKernelGGL(cg2_direction_dev_kernel, g, blk, 0, s, n, P, R, st);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

int cg2_dev_finish(int n, const double *norms, double *X, hipStream_t s)                          // X back in B's scale (cg.h:175-181)
{
  hipLaunchKernelGGL(cg2_scale_kernel, dim3(kRedBlocks), dim3(kRedThreads), 0, s, n, norms[0], norms[1], X);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

static thread_local double g_last_cg_state[kStDoubles];
static thread_local bool g_last_cg_state_set = false;

static thread_local double g_last_mscg_state[kMscgMaxShifts * kMsStride];
static thread_local int g_last_mscg_doubles = 0;

static thread_local double g_last_pcgn_state[kPcgnMaxRhs * kPnStride];
static thread_local int g_last_pcgn_doubles = 0;

// the last fs_mscgn on the calling thread: every column's st[] (fs_mscg's layout) and ms[], k and m
static thread_local std::vector<double> g_last_mscgn_cst, g_last_mscgn_ms;
static thread_local int g_last_mscgn_k = 0, g_last_mscgn_m = 0;

// the segments of the last fs_pcgn / fs_pcgn_lambdas on the calling thread: {first iteration, width, mask of original columns} each
constexpr int kPcgnMaxSegments = 8;
static thread_local int g_last_pcgn_segments[3 * kPcgnMaxSegments];
static thread_local int g_last_pcgn_nseg = 0;

static void pcgn_note_segments(const std::vector<PcgnSegment> &segs)
{
  g_last_pcgn_nseg = (int)segs.size() < kPcgnMaxSegments ? (int)segs.size() : kPcgnMaxSegments;
  for (int i = 0; i < g_last_pcgn_nseg; ++i) {
    g_last_pcgn_segments[3 * i] = segs[(size_t)i].first;
    g_last_pcgn_segments[3 * i + 1] = segs[(size_t)i].width;
    g_last_pcgn_segments[3 * i + 2] = (int)segs[(size_t)i].mask;
  }
}

void note_cg_state(const double *st_host)
{
  for (int i = 0; i < kStDoubles; ++i) g_last_cg_state[i] = st_host[i];
  g_last_cg_state_set = true;
}

// the end of an fs_pcgn solve on the host: fin = the final st[], fcs = the final cs[] of the k columns.  fs_pcg's slots of the st[]
// kept for fs_debug_last_cg_state carry column 0's scalars (with k = 1 it is fs_pcg's st[]); cs[] is kept for
// fs_debug_last_pcgn_state; info: k entries or NULL
void pcgn_note_state(const double *fin_in, const double *fcs, int k, fs_pcg_info *info)
{
  double fin[kStDoubles];
  for (int i = 0; i < kStDoubles; ++i) fin[i] = fin_in[i];
  fin[kStRsq] = fcs[kPnRz]; fin[kStAlpha] = fcs[kPnAlpha]; fin[kStBeta] = fcs[kPnBeta]; fin[kStStop] = fcs[kPnStop];
  fin[kStRr] = fcs[kPnRr]; fin[kStBb] = fcs[kPnBb];
  note_cg_state(fin);
  for (int i = 0; i < k * kPnStride; ++i) g_last_pcgn_state[i] = fcs[i];
  g_last_pcgn_doubles = k * kPnStride;
  pcgn_note_segments({PcgnSegment{0, k, pcgn_all_columns(k)}});   // a solve that narrowed says so behind this call
  for (int j = 0; info && j < k; ++j) {
    const double *e = fcs + j * kPnStride;
    info[j].iterations = (int)e[kPnCount];                   // a column still live at the cap: count = cap, converged 0
    info[j].converged = e[kPnConverged] != 0.0;
    info[j].rnorm = sqrt(e[kPnRr]);
    info[j].bnorm = sqrt(e[kPnBb]);
  }
}

// the end of an fs_mscg solve on the host: fin = the final st[] (kept for fs_debug_last_cg_state), fms = the final ms[] of the m
// shifts (kept for fs_debug_last_mscg_state); info: m entries or NULL
void mscg_note_state(const double *fin, const double *fms, int m, fs_pcg_info *info)
{
  note_cg_state(fin);
  for (int i = 0; i < m * kMsStride; ++i) g_last_mscg_state[i] = fms[i];
  g_last_mscg_doubles = m * kMsStride;
  for (int i = 0; info && i < m; ++i) {
    const double *e = fms + i * kMsStride;
    info[i].iterations = (int)e[kMsCount];                   // a shift still live at the cap: count = cap, converged 0
    info[i].converged = e[kMsConverged] != 0.0;
    info[i].rnorm = e[kMsRn];
    info[i].bnorm = sqrt(fin[kStBb]);
  }
}

// the end of an fs_mscgn solve on the host: fcst = the k columns' final st[], fms = their final ms[] (both kept for
// fs_debug_last_mscgn_state); info: m * k entries, info[i * k + j], or NULL
void mscgn_note_state(const double *fcst, const double *fms, int k, int m, fs_pcg_info *info)
{
  g_last_mscgn_cst.assign(fcst, fcst + (size_t)k * kStDoubles);
  g_last_mscgn_ms.assign(fms, fms + (size_t)k * kMscgStateDoubles);
  g_last_mscgn_k = k; g_last_mscgn_m = m;
  for (int i = 0; info && i < m; ++i)
    for (int j = 0; j < k; ++j) {
      const double *e = fms + (size_t)j * kMscgStateDoubles + i * kMsStride;
      fs_pcg_info &o = info[(size_t)i * k + j];
      o.iterations = (int)e[kMsCount];                       // a pair still live at the cap: count = cap, converged 0
      o.converged = e[kMsConverged] != 0.0;
      o.rnorm = e[kMsRn];
      o.bnorm = sqrt(fcst[(size_t)j * kStDoubles + kStBb]);
    }
}

// two ranks' final cs[]: every column ended live or not, converged or not, with the same count
bool pcgn_same_outcome(const double *a, const double *b, int k)
{
  for (int j = 0; j < k; ++j)
    for (int at : {(int)kPnLive, (int)kPnConverged, (int)kPnCount})
      if (a[j * kPnStride + at] != b[j * kPnStride + at]) return false;
  return true;
}

// two ranks' final ms[]: every shift ended live or not, converged or not, with the same count
bool mscg_same_outcome(const double *a, const double *b, int m)
{
  for (int i = 0; i < m; ++i)
    for (int at : {(int)kMsLive, (int)kMsConverged, (int)kMsCount})
      if (a[i * kMsStride + at] != b[i * kMsStride + at]) return false;
  return true;
}

int CgFlags::init()
{
  FS_HIP(hipHostMalloc((void **)&h, sizeof(double) * 4));
  h[0] = h[1] = h[2] = h[3] = 0.0;
  FS_HIP(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming));
  FS_HIP(hipEventCreateWithFlags(&ev[1], hipEventDisableTiming));
  return FS_OK;
}

CgFlags::~CgFlags()
{
  if (h) (void)hipHostFree(h);
  for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
}

int CgFlags::after_iteration(int iter, const double *st, hipStream_t s, bool *stop)
{
  FS_HIP(hipMemcpyAsync(h + 2 * (iter & 1), st + kCgStateDone, sizeof(double) * 2, hipMemcpyDeviceToHost, s));
  FS_HIP(hipEventRecord(ev[iter & 1], s));
  *stop = false;
  if (iter >= 1) {
    FS_HIP(hipEventSynchronize(ev[(iter - 1) & 1]));
    *stop = h[2 * ((iter - 1) & 1)] != 0.0;
  }
  return FS_OK;
}

}  // namespace fs

using namespace fs;

// ---- the host frame of the four single-device solvers: the shape check, fixed-order products, the work space every solve has
// (r, p, q of k F doubles, tmp of k N, part, red, st), the iterations and the final st[] on the host.  A solver brings its own
// argument checks, its own buffers (through alloc(), which keeps the order of the allocations), its start and its steps.  The
// fixed-order scope opens with the struct, before the shape check: a thread-local count that every return path gives back.
struct CgSolve {
  const char *who;
  fs_matrix_t A, At;
  int k;                                                  // right-hand sides: the products are fs_spmv (1) or fs_spmm (2)
  fs_stream_t stream;
  FixedOrderScope fixed{options().cg_fixed_order != 0};   // the products of a solve add in a fixed order: bit-identical run to run
  Workspace ws;
  CgFlags fl;
  int N = 0, F = 0;
  double *r = nullptr, *p = nullptr, *q = nullptr, *tmp = nullptr, *part = nullptr, *red = nullptr, *st = nullptr;
  double fin[kStDoubles] = {0.0};                         // the final st[], after finish()

  int shape()
  {
    N = A->a.nrow; F = A->a.ncol;
    if (At->a.nrow != F || At->a.ncol != N) { set_error(std::string(who) + ": At is not the transpose shape of A"); return FS_ERR_ARG; }
    return FS_OK;
  }
  // before anything is written to the caller's x: a solve whose products would read plain CSR arrays that fs_matrix_release_csr
  // gave back (strict_order, spmv_kernel 1-3, the row kernel of k columns) ends here and not behind its start kernels.  For
  // k >= 2 after the solver's fs_matrix_prepare calls: they settle the plan
  int ready() { return ready_for(k); }
  // the same look at the products of kk columns (option "pcgn_compact": the widths a solve may narrow to)
  int ready_for(int kk)
  {
    for (fs_matrix_t M : {A, At}) {
      if (M->a.nrow == 0) continue;
      bool plain;
      {
        std::lock_guard<std::mutex> g(M->lock);
        plain = kk == 1 ? spmv_reads_plain_csr(M->a) : spmm_reads_plain_csr(M->a, kk);
      }
      if (plain)
        if (int rc = need_plain_csr(M->a, who)) return rc;
    }
    return FS_OK;
  }
  // the work space, st[] (the scalars live on the device from the first iteration on) and the host's flags.  A solver's own
  // buffers keep their places in the order of the allocations: *own (n_own doubles) before st, *own2 behind it
  int alloc(double **own = nullptr, size_t n_own = 0, double **own2 = nullptr, size_t n_own2 = 0)
  {
    r = ws.get((size_t)k * F); p = ws.get((size_t)k * F); q = ws.get((size_t)k * F); tmp = ws.get((size_t)k * N);
    part = ws.get(kRedBlocks * 3); red = ws.get(4);
    if (own) *own = ws.get(n_own);
    st = ws.get(kStDoubles);
    if (own2) *own2 = ws.get(n_own2);
    if (!r || !p || !q || !tmp || !part || !red || !st || (own && !*own) || (own2 && !*own2)) {
      set_error(std::string(who) + ": out of device memory"); return FS_ERR_HIP;
    }
    return fl.init();
  }
  // up to cap iterations: tmp = A p, q = A' tmp, the solver's steps, the flags behind them.  look_first: a solve that is done
  // before it starts (b = 0, a warm start from a converged x) enqueues no product -- one synchronous look at the flag
  template <typename Steps>
  int iterate(int cap, bool look_first, Steps steps)
  {
    hipStream_t s = (hipStream_t)stream;
    if (look_first) {
      FS_HIP(hipMemcpyAsync(fl.h, st + kCgStateDone, sizeof(double) * 2, hipMemcpyDeviceToHost, s));
      FS_HIP(hipStreamSynchronize(s));
      if (fl.h[0] != 0.0) return FS_OK;
    }
    for (int iter = 0; iter < cap; iter++) {
      if (int rc = k == 1 ? fs_spmv(A, tmp, p, stream) : fs_spmm(A, tmp, p, k, stream)) return rc;
      if (int rc = k == 1 ? fs_spmv(At, q, tmp, stream) : fs_spmm(At, q, tmp, k, stream)) return rc;
      if (int rc = steps()) return rc;
      bool stop = false;
      if (int rc = fl.after_iteration(iter, st, s, &stop)) return rc;
      if (stop) break;
    }
    return FS_OK;
  }
  int finish()
  {
    FS_HIP(hipMemcpyAsync(fin, st, sizeof(fin), hipMemcpyDeviceToHost, (hipStream_t)stream));
    FS_HIP(hipStreamSynchronize((hipStream_t)stream));
    note_cg_state(fin);
    return FS_OK;
  }
};

// ---- option "pcgn_compact": what a narrowing solve holds besides CgSolve's work space, and its iterations ------------------------
// A panel of the solve: w columns of X, R, P; orig.v[c]: the original column of its column c, < 0: padding
struct PcgnPanel {
  int w;
  double *X, *R, *P;
  PcgnColMap orig;
};

// The narrow panels: the first, third and fifth repack go to xa, ra, pa (w1 F doubles each, w1 the widest usable rung), the second
// and fourth to xb (w2 F, the next rung) and to CgSolve's full-width r and p, which the first repack left free.  Q and the
// products' T stay in CgSolve's q and tmp at every width.  home: every column's scalars in original numbering.  h: st[0 .. 12] of
// the two most recent iterations in pinned memory -- CgFlags' look with the live mask next to `done`
constexpr int kPcgnLookDoubles = kStLiveMask + 1;
struct PcgnArena {
  double *xa = nullptr, *ra = nullptr, *pa = nullptr, *xb = nullptr, *home = nullptr, *h = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  int init(Workspace &ws, unsigned usable, int F, const char *who)
  {
    int w1 = 0, w2 = 0;
    for (int w : kPcgnRungs)
      if ((usable & (unsigned)w) != 0u) { w2 = w1; w1 = w; }
    xa = ws.get((size_t)w1 * F); ra = ws.get((size_t)w1 * F); pa = ws.get((size_t)w1 * F);
    xb = w2 ? ws.get((size_t)w2 * F) : xa;
    home = ws.get(kPcgnMaxRhs * kPnStride);
    if (!xa || !ra || !pa || !xb || !home) { set_error(std::string(who) + ": out of device memory"); return FS_ERR_HIP; }
    FS_HIP(hipHostMalloc((void **)&h, sizeof(double) * 2 * kStDoubles));
    FS_HIP(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming));
    FS_HIP(hipEventCreateWithFlags(&ev[1], hipEventDisableTiming));
    return FS_OK;
  }
  ~PcgnArena()
  {
    if (h) (void)hipHostFree(h);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  }
};

// the rungs below k a solve may narrow to, settled before anything is written to X: the one-time work of every rung's products and
// CgSolve's look at them.  A rung that answers FS_ERR_RELEASED is left out, silently; any other error ends the solve
static int pcgn_usable_rungs(CgSolve &f, unsigned *usable)
{
  *usable = 0u;
  for (int w : {16, 8, 4, 2, 1}) {
    if (w >= f.k) continue;
    int rc = FS_OK;
    if (w >= 2) {
      rc = fs_matrix_prepare(f.A, w, 0, f.stream);
      if (!rc) rc = fs_matrix_prepare(f.At, w, 0, f.stream);
    }
    if (!rc) rc = f.ready_for(w);
    if (rc == FS_ERR_RELEASED) continue;
    if (rc) return rc;
    *usable |= (unsigned)w;
  }
  return FS_OK;
}

// CgSolve::iterate for a solve that narrows.  steps(w, lambdas, X, B, R, P): everything of an iteration behind the products on a
// panel of w columns.  *end: the panel the solve ends in (X the caller's: nothing moved)
template <typename Steps>
static int pcgn_iterate_narrowing(CgSolve &f, int cap, PcgnSchedule &S, double *X, const double *B, const PcgnLambdas &lv, double *cs,
                                  PcgnArena &M, Steps steps, PcgnPanel *end)
{
  hipStream_t s = (hipStream_t)f.stream;
  const int k = f.k, F = f.F;
  double *st = f.st;
  PcgnPanel cur{k, X, f.r, f.p, {}};
  for (int c = 0; c < kPcgnMaxRhs; ++c) cur.orig.v[c] = (signed char)(c < k ? c : -1);
  *end = cur;
  FS_HIP(hipMemcpyAsync(M.h, st, sizeof(double) * kPcgnLookDoubles, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  if (M.h[kStDone] != 0.0) return FS_OK;
  auto original = [](const PcgnColMap &orig, int w, unsigned m) {          // a panel's mask in original numbering
    unsigned o = 0u;
    for (int c = 0; c < w; ++c)
      if (((m >> c) & 1u) != 0u && orig.v[c] >= 0) o |= 1u << orig.v[c];
    return o;
  };
  unsigned known = original(cur.orig, k, (unsigned)M.h[kStLiveMask]);        // m_0 = m_1; then the mask after iteration n - 2
  PcgnPanel prev = cur, ran[2] = {cur, cur};                                 // ran[n & 1]: the panel iteration n ran on
  PcgnLambdas lw = lv;
  int repacks = 0;
  for (int n = 0; n < cap; ++n) {
    const int to = S.before_iteration(n, known);
    if (to) {
      prev = cur;
      const bool first = (repacks & 1) == 0;
      PcgnPanel nx{to, first ? M.xa : M.xb, first ? M.ra : f.r, first ? M.pa : f.p, {}};
      PcgnColMap from, back;
      for (int c = 0; c < kPcgnMaxRhs; ++c) from.v[c] = back.v[c] = nx.orig.v[c] = -1;
      int at = 0;
      bool leave = false;
      for (int c = 0; c < cur.w; ++c) {
        const int o = cur.orig.v[c];
        if (o < 0) continue;
        if (((known >> o) & 1u) != 0u) { from.v[at] = (signed char)c; nx.orig.v[at] = (signed char)o; ++at; }
        else if (cur.X != X) { back.v[o] = (signed char)c; leave = true; }    // final: its x goes back to the caller's panel
      }
      if (leave)
        if (int rc = pcgn_repack_launch(true, F, cur.w, k, back, cur.X, nullptr, nullptr, X, nullptr, nullptr, st, s)) return rc;
      if (int rc = pcgn_repack_launch(false, F, cur.w, to, from, cur.X, cur.R, cur.P, nx.X, nx.R, nx.P, st, s)) return rc;
      hipLaunchKernelGGL(pcgn_remap_kernel, dim3(1), dim3(kRedThreads), 0, s, st, cs, M.home, cur.orig, from, cur.w, to, 0, 1);
      FS_HIP(hipGetLastError());
      cur = nx;
      ++repacks;
    }
    ran[n & 1] = cur;
    for (int c = 0; c < kPcgnMaxRhs; ++c) lw.v[c] = cur.orig.v[c] >= 0 ? lv.v[(int)cur.orig.v[c]] : 0.0;
    if (int rc = cur.w == 1 ? fs_spmv(f.A, f.tmp, cur.P, f.stream) : fs_spmm(f.A, f.tmp, cur.P, cur.w, f.stream)) return rc;
    if (int rc = cur.w == 1 ? fs_spmv(f.At, f.q, f.tmp, f.stream) : fs_spmm(f.At, f.q, f.tmp, cur.w, f.stream)) return rc;
    if (int rc = steps(cur.w, lw, cur.X, cur.X == X ? B : cur.X, cur.R, cur.P)) return rc;
    FS_HIP(hipMemcpyAsync(M.h + kStDoubles * (n & 1), st, sizeof(double) * kPcgnLookDoubles, hipMemcpyDeviceToHost, s));
    FS_HIP(hipEventRecord(M.ev[n & 1], s));
    if (n >= 1) {
      FS_HIP(hipEventSynchronize(M.ev[(n - 1) & 1]));
      const double *h = M.h + kStDoubles * ((n - 1) & 1);
      if (h[kStDone] != 0.0) {                              // done before iteration n: what was enqueued with it did nothing
        if (to) { S.not_run(n); cur = prev; }
        break;
      }
      known = original(ran[(n - 1) & 1].orig, ran[(n - 1) & 1].w, (unsigned)h[kStLiveMask]);
    }
  }
  *end = cur;
  return FS_OK;
}

// fs_pcgn's frame, and fs_pcgn_lambdas' (lams: k doubles on the host; lambda is not read then).  The two differ in the lambda the
// kernels take and in what FS_PRECOND_JACOBI leaves in `dinv`: the inverse of fs_gram_diag(At, lambda), or s = fs_gram_diag(At, 0)
// itself, which the per-column kernels invert as s + lambda_c per element (no pcg_dev_dinv pass)
static int pcgn_solve(const char *who, fs_matrix_t A, fs_matrix_t At, double *X, const double *B, int k, double lambda,
                      const double *lams, const fs_pcg_params *prm, fs_pcg_info *info, fs_stream_t stream)
{
  const std::string w(who);
  if (k < 1 || k > kPcgnMaxRhs) { set_error(w + ": k outside 1..FS_PCGN_MAX_RHS"); return FS_ERR_ARG; }
  CgSolve f{who, A, At, k, stream};
  if (int rc = f.shape()) return rc;
  if (int rc = pcg_params_ok(who, prm)) return rc;
  PcgnLambdas lv = {};
  for (int j = 0; lams && j < k; ++j) {
    if (!isfinite(lams[j])) { set_error(w + ": a lambda is NaN or infinite"); return FS_ERR_ARG; }
    lv.v[j] = lams[j];
  }
  if (prm->precond == FS_PRECOND_JACOBI)                     // before anything is written to X
    if (int rc = need_plain_csr(At->a, (w + " with FS_PRECOND_JACOBI (fs_gram_diag)").c_str())) return rc;
  if (k >= 2) {                                              // the k-column copies of both matrices (fs_spmm itself never builds)
    if (int rc = fs_matrix_prepare(A, k, 0, stream)) return rc;
    if (int rc = fs_matrix_prepare(At, k, 0, stream)) return rc;
  }
  if (int rc = f.ready()) return rc;
  unsigned usable = 0u;                                      // option "pcgn_compact": the rungs below k the solve may narrow to
  if (options().pcgn_compact != 0)
    if (int rc = pcgn_usable_rungs(f, &usable)) return rc;
  const bool pre = prm->precond != FS_PRECOND_NONE, warm = prm->warm_start != 0;
  const bool colj = lams && prm->precond == FS_PRECOND_JACOBI;   // the diagonal follows the column: dinv holds s
  const int F = f.F;
  const int cap = prm->max_iter > 0 ? prm->max_iter : F;     // cg.h:55
  hipStream_t s = (hipStream_t)stream;
  double *dinv = nullptr, *own = nullptr;
  const size_t npart = (size_t)kRedBlocks * 2 * k;
  if (int rc = f.alloc(pre ? &dinv : nullptr, F, &own, npart + kPcgnMaxRhs * kPnStride)) return rc;
  PcgnArena narrow;
  if (usable)
    if (int rc = narrow.init(f.ws, usable, F, who)) return rc;
  double *r = f.r, *p = f.p, *q = f.q, *st = f.st, *part = own, *cs = own + npart;
  if (int rc = pcgn_dev_clear(cs, s)) return rc;
  if (prm->precond == FS_PRECOND_JACOBI)
    if (int rc = fs_gram_diag(At, colj ? 0.0 : lambda, dinv, stream)) return rc;
  if (pre && !colj)
    if (int rc = pcg_dev_dinv(F, prm->precond == FS_PRECOND_DIAG ? prm->diag : dinv, dinv, s)) return rc;
  if (warm) {                                                // R = B - (A'(A X) + lambda X): one pair of k-column products
    if (int rc = k == 1 ? fs_spmv(A, f.tmp, X, stream) : fs_spmm(A, f.tmp, X, k, stream)) return rc;
    if (int rc = k == 1 ? fs_spmv(At, q, f.tmp, stream) : fs_spmm(At, q, f.tmp, k, stream)) return rc;
  }
  if (int rc = colj   ? pcgn_init_launch(F, k, warm, lv, B, X, r, p, q, dinv, part, st, cs, prm->tol, s, lv)
               : lams ? pcgn_init_launch(F, k, warm, lv, B, X, r, p, q, dinv, part, st, cs, prm->tol, s)
                      : pcgn_dev_init(F, k, warm, lambda, B, X, r, p, q, dinv, part, st, cs, prm->tol, s)) return rc;
  // everything of an iteration behind the products, on a panel of w columns (w = k: the caller's X, the solve's r and p)
  auto steps = [&](int w, const PcgnLambdas &lw, double *Xw, const double *Bw, double *Rw, double *Pw) {
    return colj   ? pcgn_steps_launch(F, w, lw, Xw, Bw, Rw, Pw, q, dinv, part, st, cs, s, lw)
           : lams ? pcgn_steps_launch(F, w, lw, Xw, Bw, Rw, Pw, q, dinv, part, st, cs, s)
                  : pcgn_dev_steps(F, w, lambda, Xw, Bw, Rw, Pw, q, dinv, part, st, cs, s);
  };
  PcgnSchedule sched(k, usable);
  const double *fcs_dev = cs;
  if (!usable) {
    if (int rc = f.iterate(cap, true, [&] { return steps(k, lv, X, B, r, p); })) return rc;
  } else {
    PcgnPanel end;
    if (int rc = pcgn_iterate_narrowing(f, cap, sched, X, B, lv, cs, narrow, steps, &end)) return rc;
    if (end.X != X) {                                        // the last panel's x and every column's scalars back in original numbering
      PcgnColMap back, none;
      for (int c = 0; c < kPcgnMaxRhs; ++c) back.v[c] = none.v[c] = -1;
      for (int c = 0; c < end.w; ++c)
        if (end.orig.v[c] >= 0) back.v[(int)end.orig.v[c]] = (signed char)c;
      if (int rc = pcgn_repack_launch(true, F, end.w, k, back, end.X, nullptr, nullptr, X, nullptr, nullptr, nullptr, s)) return rc;
      hipLaunchKernelGGL(pcgn_remap_kernel, dim3(1), dim3(kRedThreads), 0, s, st, cs, narrow.home, end.orig, none, end.w, 0, k, 0);
      FS_HIP(hipGetLastError());
      fcs_dev = narrow.home;
    }
  }
  double fcs[kPcgnMaxRhs * kPnStride] = {0.0};
  FS_HIP(hipMemcpyAsync(fcs, fcs_dev, sizeof(double) * k * kPnStride, hipMemcpyDeviceToHost, s));
  if (int rc = f.finish()) return rc;
  pcgn_note_state(f.fin, fcs, k, info);
  pcgn_note_segments(sched.segs);
  return FS_OK;
}

extern "C" {

// y += a x on device vectors (the "+ lambda x" of bsbm_AtA, cg.h:17-21)
int fs_axpy(int n, double a, const double *x, double *y, fs_stream_t stream)
{
  if (n < 0 || !x || !y) { set_error("fs_axpy: bad argument"); return FS_ERR_ARG; }
  hipLaunchKernelGGL(axpy_kernel, dim3(kRedBlocks), dim3(kRedThreads), 0, (hipStream_t)stream, n, a, x, y);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// (A'A + lambda I) x = b with A given by its handle and the handle of its transpose (the reference passes both
// matrices, cg.h:26-27); x, b device vectors of F = ncol(A) doubles.  Stops like cg.h:69 (||r|| <= tol ||b||) or
// after F iterations; *out_iter as the reference reports it.
int fs_cg(fs_matrix_t A, fs_matrix_t At, double *x, const double *b, double lambda, double tol, int *out_iter,
          fs_stream_t stream)
{
  FS_RANGE("fs_cg");
  if (!A || !At || !x || !b) { set_error("fs_cg: NULL argument"); return FS_ERR_ARG; }
  CgSolve f{"fs_cg", A, At, 1, stream};
  if (int rc = f.shape()) return rc;
  if (int rc = f.ready()) return rc;
  if (int rc = f.alloc()) return rc;
  const int F = f.F;
  hipStream_t s = (hipStream_t)stream;
  const CgSums sums{f.part, f.red, f.st};
  if (int rc = cg_dev_init(F, b, x, f.r, f.p, sums, tol, s)) return rc;
  if (int rc = f.iterate(F, false, [&] { return cg_dev_steps(F, lambda, x, f.r, f.p, f.q, nullptr, sums, kStepCgBeta, s); })) return rc;
  if (int rc = f.finish()) return rc;
  if (out_iter) *out_iter = (int)f.fin[kStIter];
  return FS_OK;
}

// d[j] = lambda + sum of v^2 over row j of At = the diagonal of A'A + lambda I, from the transpose handle a caller of fs_cg holds
// (the rows of A' are the columns of A: no atomics, no second pass over A).  Stream-ordered, no allocation.
int fs_gram_diag(fs_matrix_t At, double lambda, double *d, fs_stream_t stream)
{
  FS_RANGE("fs_gram_diag");
  if (!At || !d) { set_error("fs_gram_diag: NULL argument"); return FS_ERR_ARG; }
  if (int rc = need_plain_csr(At->a, "fs_gram_diag")) return rc;
  const int n = At->a.nrow, waves = kRedThreads / 64;
  // few rows per wave; 10 M rows of 16 entries take 1.3 ms (a wave per short row is what costs, not the stride: 1.4 ms with
  // 4096 workgroups) -- one-time work, about one iteration of the solve it serves
  const int blocks = n / waves + 1 < (1 << 20) ? n / waves + 1 : 1 << 20;
  hipLaunchKernelGGL(gram_diag_kernel, dim3(blocks), dim3(kRedThreads), 0, (hipStream_t)stream, n, At->a.row_ptr, At->a.vals, lambda, d);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// (A'A + lambda I) x = b by conjugate gradients with a diagonal preconditioner, a warm start and an iteration cap: see
// include/fastsparse_hip.h for the arithmetic.  Without a preconditioner, from a cold start and with the cap at F, the iterations
// launch fs_cg's own kernels on the same data (the scalar step of the convergence test also keeps r.r and b.b for fs_pcg_info).
int fs_pcg(fs_matrix_t A, fs_matrix_t At, double *x, const double *b, double lambda, const fs_pcg_params *prm, fs_pcg_info *info,
           fs_stream_t stream)
{
  FS_RANGE("fs_pcg");
  if (!A || !At || !x || !b || !prm) { set_error("fs_pcg: NULL argument"); return FS_ERR_ARG; }
  CgSolve f{"fs_pcg", A, At, 1, stream};
  if (int rc = f.shape()) return rc;
  if (int rc = pcg_params_ok("fs_pcg", prm)) return rc;
  if (prm->precond == FS_PRECOND_JACOBI)                     // before anything is written to x
    if (int rc = need_plain_csr(At->a, "fs_pcg with FS_PRECOND_JACOBI (fs_gram_diag)")) return rc;
  if (int rc = f.ready()) return rc;
  const bool pre = prm->precond != FS_PRECOND_NONE, warm = prm->warm_start != 0;
  const int F = f.F;
  const int cap = prm->max_iter > 0 ? prm->max_iter : F;     // cg.h:55
  hipStream_t s = (hipStream_t)stream;
  double *dinv = nullptr;
  if (int rc = f.alloc(pre ? &dinv : nullptr, F)) return rc;
  double *r = f.r, *p = f.p, *q = f.q;
  const CgSums sums{f.part, f.red, f.st};
  if (prm->precond == FS_PRECOND_JACOBI)
    if (int rc = fs_gram_diag(At, lambda, dinv, stream)) return rc;
  if (pre)
    if (int rc = pcg_dev_dinv(F, prm->precond == FS_PRECOND_DIAG ? prm->diag : dinv, dinv, s)) return rc;
  if (warm) {                                                // r = b - (A'(A x) + lambda x)
    if (int rc = fs_spmv(A, f.tmp, x, stream)) return rc;
    if (int rc = fs_spmv(At, q, f.tmp, stream)) return rc;
  }
  if (int rc = pcg_dev_init(F, warm, lambda, b, x, r, q, sums, prm->tol, s)) return rc;            // b.b, r.r, stop, done?
  if (int rc = pcg_dev_start(F, r, dinv, p, sums, s)) return rc;                                   // p = z, r.z
  if (int rc = f.iterate(cap, true, [&] { return cg_dev_steps(F, lambda, x, r, p, q, dinv, sums, kStepPcgBeta, s); })) return rc;
  if (int rc = f.finish()) return rc;
  pcg_info_of(f.fin, info);
  return FS_OK;
}

// (A'A + lambda[i] I) x_i = b for i < m by multi-shift conjugate gradients: one Krylov sequence on the smallest lambda, two products
// per iteration whatever m is; see include/fastsparse_hip.h for the arithmetic.  The base system's steps are fs_cg's (its kernels
// for q += base p and the partial sums' shape for r.r), so the columns of the smallest lambda have fs_cg's bits.
int fs_mscg(fs_matrix_t A, fs_matrix_t At, double *X, int64_t ldx, const double *b, int m, const double *lambda, double tol,
            int max_iter, fs_pcg_info *info, fs_stream_t stream)
{
  FS_RANGE("fs_mscg");
  if (!A || !At || !X || !b || !lambda) { set_error("fs_mscg: NULL argument"); return FS_ERR_ARG; }
  CgSolve f{"fs_mscg", A, At, 1, stream};
  if (int rc = f.shape()) return rc;
  const int F = f.F;
  if (int rc = mscg_args_ok("fs_mscg", F, ldx, m, lambda, tol)) return rc;
  if (int rc = f.ready()) return rc;
  const MscgShifts sh = mscg_shifts(m, lambda);
  const int cap = max_iter > 0 ? max_iter : F;               // cg.h:55
  const long long ldp = ((long long)F + 1) & ~1LL;           // every P_i 16-byte aligned
  hipStream_t s = (hipStream_t)stream;
  double *P = nullptr, *ms = nullptr;
  if (int rc = f.alloc(&P, (size_t)ldp * sh.nslots, &ms, kMscgMaxShifts * kMsStride)) return rc;
  double *r = f.r, *p = f.p, *q = f.q;
  const CgSums sums{f.part, f.red, f.st};
  const MscgScalars K{ms, m, tol, &sh};
  if (int rc = mscg_dev_init(F, b, r, p, X, (long long)ldx, P, ldp, sums, K, s)) return rc;
  if (int rc = f.iterate(cap, true, [&] { return mscg_dev_steps(F, sh.base, r, p, q, X, (long long)ldx, P, ldp, sums, K, s); })) return rc;
  double fms[kMscgMaxShifts * kMsStride] = {0.0};
  FS_HIP(hipMemcpyAsync(fms, ms, sizeof(double) * m * kMsStride, hipMemcpyDeviceToHost, s));
  if (int rc = f.finish()) return rc;
  mscg_note_state(f.fin, fms, m, info);
  return FS_OK;
}

// (A'A + lambda[i] I) x_ij = b_j for i < m, j < k: fs_mscg on every column of B, on one pair of k-column products per iteration;
// see include/fastsparse_hip.h for what differs from fs_mscg.  The per-column sums are formed by fs_pcgn's kernels, the scalar
// steps are fs_mscg's, so column j of panel i has the bits of fs_mscg's x_i on B[:, j] wherever the k-column product has the
// single-vector product's bits, and with m = 1 the solve is fs_pcgn without a preconditioner from a cold start.
int fs_mscgn(fs_matrix_t A, fs_matrix_t At, double *X, int64_t ldx, const double *B, int k, int m, const double *lambda, double tol,
             int max_iter, fs_pcg_info *info, fs_stream_t stream)
{
  FS_RANGE("fs_mscgn");
  if (!A || !At || !X || !B || !lambda) { set_error("fs_mscgn: NULL argument"); return FS_ERR_ARG; }
  if (k < 1 || k > kPcgnMaxRhs) { set_error("fs_mscgn: k outside 1..FS_PCGN_MAX_RHS"); return FS_ERR_ARG; }
  CgSolve f{"fs_mscgn", A, At, k, stream};
  if (int rc = f.shape()) return rc;
  const int F = f.F;
  if (ldx < (int64_t)F * k) { set_error("fs_mscgn: ldx < ncol(A) * k"); return FS_ERR_ARG; }
  if (int rc = mscg_args_ok("fs_mscgn", 0, ldx, m, lambda, tol)) return rc;     // (ldx is settled above)
  if (k >= 2) {                                              // the k-column copies of both matrices (fs_spmm itself never builds)
    if (int rc = fs_matrix_prepare(A, k, 0, stream)) return rc;
    if (int rc = fs_matrix_prepare(At, k, 0, stream)) return rc;
  }
  if (int rc = f.ready()) return rc;
  const MscgShifts sh = mscg_shifts(m, lambda);
  const int cap = max_iter > 0 ? max_iter : F;               // cg.h:55
  const size_t ne = (size_t)F * k;
  const long long ldp = (long long)((ne + 1) & ~(size_t)1);  // every P_i 16-byte aligned
  hipStream_t s = (hipStream_t)stream;
  const size_t npart = pcgn_part_doubles(k), nscal = kPcgnSendDoubles + kPcgnStateDoubles + (size_t)kPcgnMaxRhs * kStDoubles +
                                                     kMscgnStateDoubles + kMscgnListDoubles;
  double *Ps = nullptr, *own = nullptr;
  if (int rc = f.alloc(&Ps, (size_t)ldp * sh.nslots, &own, npart + nscal)) return rc;   // all of it before the first store to X
  double *part = own, *red = part + npart, *cs = red + kPcgnSendDoubles, *cst = cs + kPcgnStateDoubles;
  double *ms = cst + (size_t)kPcgnMaxRhs * kStDoubles, *sl = ms + kMscgnStateDoubles;
  FS_HIP(hipMemsetAsync(red, 0, sizeof(double) * nscal, s));  // slots a column never writes read as 0 in the debug getter
  const PcgnSums U{part, f.st, cs, red};
  const MscgnScalars K{red, cst, ms, sl, m, tol, &sh};
  if (int rc = mscgn_dev_init(F, k, B, X, (long long)ldx, f.r, f.p, f.q, Ps, ldp, U, K, s)) return rc;
  if (int rc = f.iterate(cap, true, [&] { return mscgn_dev_steps(F, k, X, (long long)ldx, f.r, f.p, f.q, Ps, ldp, U, K, s); })) return rc;
  std::vector<double> fcst((size_t)k * kStDoubles), fms((size_t)k * kMscgStateDoubles);
  FS_HIP(hipMemcpyAsync(fcst.data(), cst, sizeof(double) * fcst.size(), hipMemcpyDeviceToHost, s));
  FS_HIP(hipMemcpyAsync(fms.data(), ms, sizeof(double) * fms.size(), hipMemcpyDeviceToHost, s));
  if (int rc = f.finish()) return rc;
  mscgn_note_state(fcst.data(), fms.data(), k, m, info);
  return FS_OK;
}

// (A'A + lambda I) X = B for k right-hand sides, X and B row-major F x k: k independent fs_pcg recurrences on shared k-column
// products; see include/fastsparse_hip.h for the arithmetic.  Column j has the bits of fs_pcg on B[:, j] wherever the k-column
// product has the bits of the single-vector one ("strict_order"; k = 1 in every mode: the products are fs_spmv).
int fs_pcgn(fs_matrix_t A, fs_matrix_t At, double *X, const double *B, int k, double lambda, const fs_pcg_params *prm,
            fs_pcg_info *info, fs_stream_t stream)
{
  FS_RANGE("fs_pcgn");
  if (!A || !At || !X || !B || !prm) { set_error("fs_pcgn: NULL argument"); return FS_ERR_ARG; }
  return pcgn_solve("fs_pcgn", A, At, X, B, k, lambda, nullptr, prm, info, stream);
}

// (A'A + lambda[j] I) x_j = b_j for j < k: fs_pcgn with a lambda per column, and under FS_PRECOND_JACOBI a diagonal per column.
// Column j has the bits of fs_pcg at lambda[j] where fs_pcgn's column has those of fs_pcg; with equal lambdas it is fs_pcgn.
int fs_pcgn_lambdas(fs_matrix_t A, fs_matrix_t At, double *X, const double *B, int k, const double *lambda, const fs_pcg_params *prm,
                    fs_pcg_info *info, fs_stream_t stream)
{
  FS_RANGE("fs_pcgn_lambdas");
  if (!A || !At || !X || !B || !prm || !lambda) { set_error("fs_pcgn_lambdas: NULL argument"); return FS_ERR_ARG; }
  return pcgn_solve("fs_pcgn_lambdas", A, At, X, B, k, 0.0, lambda, prm, info, stream);
}

// two right-hand sides, X and B row-major F x 2 (cg.h:85-187)
int fs_cg2(fs_matrix_t A, fs_matrix_t At, double *X, const double *B, double lambda, double tol, int *out_iter,
           fs_stream_t stream)
{
  FS_RANGE("fs_cg2");
  if (!A || !At || !X || !B) { set_error("fs_cg2: NULL argument"); return FS_ERR_ARG; }
  CgSolve f{"fs_cg2", A, At, 2, stream};
  if (int rc = f.shape()) return rc;
  // the two-column copies of both matrices, before the first iteration (fs_spmm itself never builds)
  if (int rc = fs_matrix_prepare(A, 2, 0, stream)) return rc;
  if (int rc = fs_matrix_prepare(At, 2, 0, stream)) return rc;
  if (int rc = f.ready()) return rc;
  if (int rc = f.alloc()) return rc;
  const int F = f.F;
  hipStream_t s = (hipStream_t)stream;
  double norms[2];
  if (int rc = cg2_dev_init(F, B, X, f.r, f.p, f.part, f.red, f.st, tol, norms, s)) return rc;
  if (int rc = f.iterate(F, false, [&] { return cg2_dev_steps(F, lambda, X, f.r, f.p, f.q, f.part, f.red, f.st, s); })) return rc;
  if (int rc = cg2_dev_finish(F, norms, X, s)) return rc;
  if (int rc = f.finish()) return rc;
  if (out_iter) *out_iter = (int)f.fin[kStIter];
  return FS_OK;
}

// the final st[] (kCgStateDoubles doubles, layout of the enum above final_step_kernel) of the last solve on the calling thread:
// fs_cg / fs_cg2, or rank 0's of fs_dist_cg / fs_dist_cg2.  Returns the number of doubles written, 0 before the first solve.
// Diagnostics, not in include/fastsparse_hip.h.
int fs_debug_last_cg_state(double *out)
{
  if (!out) { set_error("fs_debug_last_cg_state: NULL argument"); return FS_ERR_ARG; }
  if (!g_last_cg_state_set) return 0;
  for (int i = 0; i < kStDoubles; ++i) out[i] = g_last_cg_state[i];
  return kStDoubles;
}

// the final per-shift array of the last fs_mscg (or rank 0's of the last fs_dist_mscg) on the calling thread: m * kMsStride doubles (layout of the kMs enum), at most
// max_doubles of them.  Returns the number of doubles written, 0 before the first solve.  Diagnostics, not in the header.
int fs_debug_last_mscg_state(double *out, int max_doubles)
{
  if (!out || max_doubles < 0) { set_error("fs_debug_last_mscg_state: bad argument"); return FS_ERR_ARG; }
  const int n = g_last_mscg_doubles < max_doubles ? g_last_mscg_doubles : max_doubles;
  for (int i = 0; i < n; ++i) out[i] = g_last_mscg_state[i];
  return n;
}

// column `column` of the last fs_mscgn on the calling thread in fs_mscg's own layouts: st (kCgStateDoubles doubles) as
// fs_debug_last_cg_state hands out fs_mscg's, ms (m * kMsStride doubles, at most max_ms_doubles of them) as fs_debug_last_mscg_state
// does.  Returns m * kMsStride, 0 before the first solve.  Diagnostics, not in the header.
int fs_debug_last_mscgn_state(int column, double *st, double *ms, int max_ms_doubles)
{
  if (!st || !ms || max_ms_doubles < 0) { set_error("fs_debug_last_mscgn_state: bad argument"); return FS_ERR_ARG; }
  if (g_last_mscgn_k == 0) return 0;
  if (column < 0 || column >= g_last_mscgn_k) { set_error("fs_debug_last_mscgn_state: no such column"); return FS_ERR_ARG; }
  for (int i = 0; i < kStDoubles; ++i) st[i] = g_last_mscgn_cst[(size_t)column * kStDoubles + i];
  const int n = g_last_mscgn_m * kMsStride < max_ms_doubles ? g_last_mscgn_m * kMsStride : max_ms_doubles;
  for (int i = 0; i < n; ++i) ms[i] = g_last_mscgn_ms[(size_t)column * kMscgStateDoubles + i];
  return g_last_mscgn_m * kMsStride;
}

// the segments of the last fs_pcgn / fs_pcgn_lambdas on the calling thread (option "pcgn_compact"): three ints per segment -- its first
// iteration, its width, the mask of the original columns its panel holds -- for at most max_segments of them.  Returns the number
// of segments, 0 before the first solve; one segment (0, k, all columns) when nothing moved.  Diagnostics, not in the header.
int fs_debug_last_pcgn_segments(int *out, int max_segments)
{
  if (!out || max_segments < 0) { set_error("fs_debug_last_pcgn_segments: bad argument"); return FS_ERR_ARG; }
  for (int i = 0; i < 3 * (g_last_pcgn_nseg < max_segments ? g_last_pcgn_nseg : max_segments); ++i) out[i] = g_last_pcgn_segments[i];
  return g_last_pcgn_nseg;
}

// the final per-column array of the last fs_pcgn on the calling thread: k * kPnStride doubles (layout of the kPn enum), at most
// max_doubles of them; a slot its column never wrote (rz, alpha of a column that is done at the start; beta before a second
// iteration) is 0.  Returns the number of doubles written, 0 before the first solve.  Diagnostics, not in the header.
int fs_debug_last_pcgn_state(double *out, int max_doubles)
{
  if (!out || max_doubles < 0) { set_error("fs_debug_last_pcgn_state: bad argument"); return FS_ERR_ARG; }
  const int n = g_last_pcgn_doubles < max_doubles ? g_last_pcgn_doubles : max_doubles;
  for (int i = 0; i < n; ++i) out[i] = g_last_pcgn_state[i];
  return n;
}

}  // extern "C"
