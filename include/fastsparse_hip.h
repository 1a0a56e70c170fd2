/*
 * fastsparse_hip.h -- C-ABI of libfastsparse_hip.so (MI355X / gfx950).
 *
 * Two layers, both plain C (no C++/torch types cross this boundary):
 *
 *  (1) the reference's own entry points -- A_mul_B, At_mul_B, csr_A_mul_B, bcsr_*,
 *      bsbm_*, sdm_*, bsdm_*, cbcsr_* and the format constructors -- declared in
 *      include/sparse.h, dsparse.h, csr.h, cbcsr.h with the reference's struct layouts
 *      and signatures.  They accept host OR device pointers for x / y and keep a
 *      device copy of each matrix in a side table keyed by the host struct
 *      (fs_invalidate / fs_release below manage that table).
 *
 *  (2) the device-resident layer declared here: opaque matrix handles living in HBM,
 *      products on device pointers and an explicit HIP stream.  This is what a
 *      device-resident caller (CG loop, multi-GPU driver, bench.py) binds, and what
 *      layer (1) is implemented on.
 *
 * Every function that can fail returns 0 on success and a negative fs_status
 * otherwise; fs_last_error() gives the message for the calling thread.  There is no
 * CPU fallback anywhere: without a usable HIP device the calls fail.
 *
 * Reference interfaces replaced (all in /root/reference):
 *   csr_A_mul_B csr.h:425, csr_A_mul_Bn csr.h:441, bcsr_A_mul_B csr.h:149,
 *   bcsr_A_mul_B2/_B4/_B8/_B8_auto/_Bn/_B32n csr.h:164-302, bcsr_AA_mul_B csr.h:305,
 *   parallel_bcsr_AA_mul_B csr.h:323, A_mul_B sparse.h:58, At_mul_B sparse.h:68,
 *   bsbm_A_mul_B/_B2/_B4/_Bn sparse.h:259-336, sdm_A_mul_B dsparse.h:43,
 *   sdm_At_mul_B dsparse.h:54, bsdm_A_mul_B dsparse.h:176, cbcsr_A_mul_B cbcsr.h:76.
 */
#ifndef FASTSPARSE_HIP_H
#define FASTSPARSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fs_matrix_s *fs_matrix_t;   /* device-resident sparse matrix (CSR, valued or pattern-only) */
typedef struct fs_cbcsr_s  *fs_cbcsr_t;    /* device-resident column-blocked binary CSR (cbcsr.h:5-14)   */
typedef void *fs_stream_t;                 /* a hipStream_t; NULL = the legacy default stream            */
typedef struct fs_dist_s *fs_dist_t;              /* the GPUs of one node as one context (one process, N devices, RCCL) */
typedef struct fs_dist_matrix_s *fs_dist_matrix_t; /* a CSR row-sharded over the devices of an fs_dist_t              */

enum fs_status {
  FS_OK = 0,
  FS_ERR_HIP = -1,        /* a HIP runtime call failed (message has the HIP error string) */
  FS_ERR_ARG = -2,        /* bad argument (NULL handle, negative size, k < 1, ...)          */
  FS_ERR_NO_DEVICE = -3,  /* no gfx950 device visible                                        */
  FS_ERR_NO_TRANSPOSE = -4, /* transposed product asked for before fs_matrix_build_transpose */
  FS_ERR_RELEASED = -5     /* the operation reads the plain CSR arrays, which fs_matrix_release_csr gave back (products that run on
                            * them, fs_matrix_download, fs_gram_diag and fs_pcg with FS_PRECOND_JACOBI, ...: see there) */
};

enum fs_memspace { FS_HOST = 0, FS_DEVICE = 1 };

/* ---- runtime ---------------------------------------------------------------------- */
const char *fs_version(void);
const char *fs_last_error(void);
int  fs_device_count(void);
int  fs_set_device(int device);
/* option names: "strict_order" (0/1: storage-order sums, bit-identical to the strict-IEEE CPU order for
 * arbitrary x), "spmv_kernel" (0 = auto, 1 streaming, 2 lanes-per-row, 6 tiled, 7 two-pass, 8 LDS-staged
 * tiled), "tiling" (0 never build the L2-tiled copy, 1 build it when the estimates do not rule it out and let the
 * builder's timing of the candidates decide, 2 always; read when a matrix is created), "tile_rows" / "tile_cols"
 * (0 = auto), "binning" and "ldsx" (the same three values for the two-pass copy and the LDS-staged tiled copy), "reproducible" (0/1, default 0: with 1 only kernels whose
 * sums are bit-identical from run to run are used -- the two-pass kernels add a row's terms with LDS atomics in
 * arrival order, so their last bits can differ between runs for non-integer data; read when a matrix is created
 * and at every product).
 * Options are process-wide.
 *
 * Threads and streams: every entry point may be called from several host threads; launches on one handle are serialised by
 * a lock.  A handle keeps scratch vectors for some kernels (rows that cross chunks in the streaming kernel, sums of cut rows in
 * the tiled kernel, the products of the two-pass kernels for k = 1 and for the k-column sweeps k = 2..4, the cell sums of a
 * column-blocked matrix, the column-major copies of X and Y of multi-column products on the LDS-staged copy, k = 2..16), so
 * products on ONE handle must not overlap in time on different streams: order them, or use one handle per stream.  Only the
 * row kernel (option "spmm_kernel" = 1; k >= 5 on matrices that keep the two-pass copy, k > 16 otherwise) and distinct handles
 * are unrestricted.  (fs_spmv_host / fs_spmv_t_host order themselves behind the handle's last device-vector product.)
 * Options are read at the call, on the calling thread, without a lock: set them before other threads create or multiply.
 * "spmm_kernel" (multi-column products: 0 auto, 1 row kernel, 2 k-column two-pass sweep for k = 2..4, 3 one single-vector sweep
 * per column, 4 the v_mfma_f64_16x16x4_f64 experiment; "strict_order" wins over every choice: its products run on the row
 * kernel, 4 included, whose fused multiply-adds would break the storage-order bits), "ata_kernel" (fs_ata_mul: 0 two products,
 * 2 the fused single kernel),
 * "device_build" (format constructors: 0 host loops, 1 on the device from 4 M entries, 2 on the device always).
 * "tile_split": rows longer than this are cut into virtual rows in the tiled copy (0 = 256).
 * "cg_fixed_order" (default 1; FS_CG_FIXED_ORDER): fs_cg / fs_cg2 / fs_dist_cg run their products with fixed-order sums, as under
 * "reproducible", so that a solve is bit-identical from run to run like the reference's loops (cg.h:25-187); 0 = the default kernels.
 * "pcgn_kernel": fs_pcgn's per-iteration vector kernels, 0 = auto (see fs_pcgn), 1 = a lane per row, 2 = the 256-row panels staged
 * through LDS with coalesced accesses; both give the same bits.
 * "pcgn_compact" (default 0; FS_PCGN_COMPACT): fs_pcgn and fs_pcgn_lambdas, 1 = the live columns of a solve move into a narrower
 * panel whenever they fit the next of the widths 16, 8, 4, 2, 1, and the products run at that width (see fs_pcgn, "Narrowing");
 * 0 = every iteration runs on all k columns.  fs_dist_pcgn, fs_dist_pcgn_lambdas and fs_mscgn do not read it.
 * "dist_cg_scheme" (FS_DIST_CG_SCHEME): fs_dist_cg, fs_dist_pcg, fs_dist_mscg and fs_dist_mscgn, 0 every device keeps whole vectors, 1 every device keeps its slice (see there). */
int  fs_set_option(const char *name, int value);
int  fs_get_option(const char *name);

/* ---- dense vectors in HBM (thin wrappers over hipMalloc/hipMemcpy for C callers without HIP headers) */
void *fs_device_alloc(int64_t bytes);
void  fs_device_free(void *p);
int   fs_copy_to_device(void *dst_dev, const void *src_host, int64_t bytes);
int   fs_copy_to_host(void *dst_host, const void *src_dev, int64_t bytes);
int   fs_device_synchronize(void);

/* ---- matrices in HBM ---------------------------------------------------------------- */
/* CSR arrays -> handle.  vals == NULL makes a pattern-only (BinaryCSR) matrix.
 * space says where row_ptr/cols/vals live.  With space == FS_DEVICE and borrow != 0 the
 * handle uses the caller's device arrays in place (they must outlive the handle and be
 * 16-byte aligned); otherwise the arrays are copied.  replaces: struct CSR csr.h:358-366,
 * struct BinaryCSR csr.h:15-22 as device-side containers. */
fs_matrix_t fs_csr_create(int nrow, int ncol, int64_t nnz, const int *row_ptr, const int *cols,
                          const double *vals, int space, int borrow);
/* COO arrays -> handle; entries are stably ordered by row on the device, so every row keeps
 * the caller's entry order (what new_csr csr.h:375-422 / new_bcsr csr.h:30-67 produce and
 * what the serial COO loops sparse.h:58-65 / dsparse.h:43-51 sum in). */
fs_matrix_t fs_coo_create(int nrow, int ncol, int64_t nnz, const int *rows, const int *cols,
                          const double *vals, int space);
void fs_matrix_destroy(fs_matrix_t A);
/* builds and caches the stably column-ordered CSR of A' (needed by *_t products) */
int  fs_matrix_build_transpose(fs_matrix_t A, fs_stream_t stream);
int  fs_matrix_has_transpose(fs_matrix_t A);
/* which kernel fs_spmv (or fs_spmv_t) runs on this matrix under the current options: 1 chunk-streaming,
 * 2 lanes-per-row, 6 L2-tiled, 7 two-pass, 8 LDS-staged tiled; the choice is made by the format builder when the matrix is created */
int  fs_matrix_spmv_kernel(fs_matrix_t A, int transposed);
/* what the format builder measured when it made that choice: ms per product (median of 5 runs on a zero vector) of
 * [0] the chunk-streaming kernel, [1] the L2-tiled kernel, [2] the LDS-staged tiled kernel, [3] the two-pass pair;
 * 0 for a candidate that was not built (ruled out by the estimates, or the matrix is small) */
int  fs_matrix_candidate_ms(fs_matrix_t A, int transposed, float *ms4);
/* where the one-time work of the matrix (transposed != 0: of its A') went, ms of host wall time: [0] arrays into HBM + validation,
 * [1] ordering (COO -> CSR; the transpose), [2] chunk schedule, [3] two-pass copy built, [4] L2-tiled copy built, [5] LDS-staged copy
 * built, [6] candidates timed, [7] losers freed + scratch trimmed.  The reference's one-time step is new_csr / new_bcsr (csr.h:375-422,
 * 30-67); fs_matrix_device_bytes says what the result holds. */
int  fs_matrix_build_ms(fs_matrix_t A, int transposed, float *ms8);
int  fs_matrix_nrow(fs_matrix_t A);
int  fs_matrix_ncol(fs_matrix_t A);
int64_t fs_matrix_nnz(fs_matrix_t A);
/* HBM bytes one product has to move at least (SURVEY.md 8d formula):
 * (12 or 4)*nnz + 4*(nrow+1) + 8*k*nrow + 8*k*ncol */
int64_t fs_matrix_algorithmic_bytes(fs_matrix_t A, int k);
/* copy the device CSR back (any pointer may be NULL); used by tests */
int  fs_matrix_download(fs_matrix_t A, int transposed, int *row_ptr, int *cols, double *vals);

/* ---- products on device pointers ---------------------------------------------------- */
/* y[nrow] = A x[ncol]           (csr_A_mul_B / bcsr_A_mul_B / A_mul_B / sdm_A_mul_B / bsbm / bsdm) */
int fs_spmv(fs_matrix_t A, double *y, const double *x, fs_stream_t stream);
/* y[ncol] = A' x[nrow]          (At_mul_B / sdm_At_mul_B; CSR At_mul_B of BASELINE config 2) */
int fs_spmv_t(fs_matrix_t A, double *y, const double *x, fs_stream_t stream);
/* The same product in nparts parts (1..64), for callers that ship finished rows while the rest still computes -- the
 * all-gather of the y shards of a row-sharded product overlapped with the product (csr.h:429: the row loop that shards).
 * Call with part = 0 .. nparts-1 in order on ONE stream; once the stream has passed part p, rows [rows[p], rows[p+1]) of y
 * are final, where rows[0 .. nparts] comes from fs_spmv_part_rows (fixed for a handle, nparts and the current options:
 * the product is cut where its kernel finishes rows anyway -- panels of pass 2 of the two-pass pair, generations of
 * workgroups of the tiled kernels; a kernel that cannot be cut does everything with part 0 and reports rows = {0, nrow,
 * nrow, ...}).  All parts together are exactly fs_spmv / fs_spmv_t.
 * The cuts of a (handle, nparts, kernel) are computed on first use -- a small synchronous download of the panel tables -- and kept
 * (the eight most recent): call fs_spmv_part_rows once before a timed or captured loop; fs_spmv_part itself then only launches. */
int fs_spmv_part_rows(fs_matrix_t A, int transposed, int nparts, int *rows /* nparts + 1 */);
int fs_spmv_part(fs_matrix_t A, int transposed, double *y, const double *x, int part, int nparts, fs_stream_t stream);
/* the same for k row-major columns (fs_spmm / fs_spmm_t in parts: the block-CG iteration): the one-sweep kernel of k = 2, 4 is cut
 * like the single-vector pair, every other plan does everything with part 0; k = 1 is fs_spmv_part */
int fs_spmm_part_rows(fs_matrix_t A, int transposed, int k, int nparts, int *rows /* nparts + 1 */);
int fs_spmm_part(fs_matrix_t A, int transposed, double *Y, const double *X, int k, int part, int nparts, fs_stream_t stream);
/* dst[dst_off[i] + j] = src[src_off[i] + j] for j < count[i], i < nseg, in one launch; table_dev = int64[3 * nseg] in HBM:
 * dst_off[nseg], src_off[nseg], count[nseg]; max_count = the largest count (sizes the grid).  Unpacks the padded receive
 * buffer of an all-gather of unequal y shards. */
int fs_copy_segments(int nseg, const int64_t *table_dev, int64_t max_count, const double *src, double *dst, fs_stream_t stream);
/* Y[nrow,k] = A X[ncol,k], X and Y row-major  (csr_A_mul_Bn, bcsr_A_mul_B2..._B32n, bsbm_A_mul_B2/_B4/_Bn).
 * Stream-ordered like fs_spmv: a product never builds a copy and never waits for the device.  What a given k can use
 * beyond the copies made at creation -- the k-column two-pass copy (k = 2..4), the measured choice between one sweep per
 * column and the row kernel (LDS-staged copy, k = 3..16) -- is made by fs_matrix_prepare; without it the product runs on
 * what the handle already holds (fs_matrix_spmm_plan tells which kernel that is). */
int fs_spmm(fs_matrix_t A, double *Y, const double *X, int k, fs_stream_t stream);
int fs_spmm_t(fs_matrix_t A, double *Y, const double *X, int k, fs_stream_t stream);
/* One-time work for products with k columns on A (transposed != 0: on A', after fs_matrix_build_transpose): builds the
 * k-column two-pass copy (k = 2, 3, 4 on matrices that keep the two-pass copy: +(4.25 + 8 kw [+ 8]) bytes per padded entry
 * of HBM with kw = 2 for k = 2, 3 and 4 for k = 4, fs_matrix_device_bytes reports it;
 * 30-40 ms at 160 M entries), allocates the column-major scratch and times column sweeps against the row kernel (k = 3..16
 * on matrices that keep the LDS-staged copy).  Synchronous; idempotent; k = 1 and k > 16 need nothing.  The drop-in
 * layer calls it on the first product with a new k, and for every k listed in the environment variable FS_PREPARE_K
 * (e.g. "2,4") when it makes the device copy of a matrix, so that no later product call carries the work. */
int fs_matrix_prepare(fs_matrix_t A, int k, int transposed, fs_stream_t stream);
/* which kernel fs_spmm / fs_spmm_t runs for this k right now: 1 row kernel, 2 k-column two-pass sweep, 3 one
 * single-vector two-pass sweep per column, 4 MFMA experiment, 5 column-major sweeps of the LDS-staged kernel, 6 / 7 strided
 * sweeps of the LDS-staged / L2-tiled kernel */
int fs_matrix_spmm_plan(fs_matrix_t A, int k, int transposed);
/* HBM the handle holds (A and, once built, A'), in bytes: [0] the CSR arrays it owns + chunk schedule, [1] the kept
 * single-vector copy (two-pass incl. its product stream / L2-tiled / LDS-staged), [2] k-column copies and multi-column scratch */
int fs_matrix_device_bytes(fs_matrix_t A, int64_t *bytes3);
/* Give back what the handle no longer needs.  fs_matrix_release_csr: once the format builder has KEPT a re-ordered copy (two-pass,
 * LDS-staged or L2-tiled) the products run on it alone; the plain row_ptr / cols / vals -- owned arrays are freed, borrowed arrays
 * are forgotten so that the caller may free them -- and the chunk schedule are dead weight (config 2: 1.96 of 5.3 GB; a config-5
 * shard: 4.8 of 12.9 GB).  Applies to A and, when built, A'; returns the number of sides released (0: no kept copy, nothing done).
 * What still needs the plain arrays afterwards fails with FS_ERR_RELEASED: strict_order and spmv_kernel 1 / 2 / 3 products, the row
 * kernel of multi-column products (k >= 5 on two-pass matrices, k > 16), fs_matrix_prepare for a new k, fs_matrix_build_transpose,
 * fs_matrix_download, the fused A'A kernel, fs_gram_diag (and with it fs_pcg with FS_PRECOND_JACOBI), and option "reproducible" on an
 * LDS-staged copy that is not orderable.
 * fs_matrix_restore_csr hands the same arrays back (same meaning of space / borrow as fs_csr_create; they are NOT validated or
 * compared again) -- "rebuild on demand" is the caller's: the re-ordered copies do not keep the storage order of a row.
 * Option "release_csr" (FS_RELEASE_CSR, default 0) = 1 releases at the end of fs_csr_create / fs_coo_create /
 * fs_matrix_build_transpose; the drop-in layer never releases (its callers keep the host arrays, and call any entry point next).
 * fs_matrix_release_prepared: the k-column copy and scratch fs_matrix_prepare made for k (0: for every k), on A and A'. */
int fs_matrix_release_csr(fs_matrix_t A);
int fs_matrix_restore_csr(fs_matrix_t A, int transposed, const int *row_ptr, const int *cols, const double *vals, int space, int borrow);
int fs_matrix_release_prepared(fs_matrix_t A, int k);
/* y[ncol] = A'A x[ncol]; tmp is caller scratch of nrow doubles in HBM   (bcsr_AA_mul_B, parallel_bcsr_AA_mul_B) */
int fs_ata_mul(fs_matrix_t A, double *y, const double *x, double *tmp, fs_stream_t stream);

/* ---- products on HOST vectors (what a caller of the reference's csr_A_mul_B(y, A, x) holds: csr.h:149) -----
 * Synchronous: y_host is complete on return.  The handle keeps its own staging vectors, stream and events.  With a
 * two-pass copy (the default for large x) x goes up band range by band range and y comes down panel range by panel
 * range while the kernels of the other ranges run (FS_HOST_CHUNKS ranges, default 8; 1 = copy, product, copy); the
 * panel kernels are launched in ranges of workgroups with y coming down behind each (tall matrices) or, when chunks
 * share panels (few long rows), with x going up in the ranges the launch order needs. */
int fs_spmv_host(fs_matrix_t A, double *y_host, const double *x_host);
int fs_spmv_t_host(fs_matrix_t A, double *y_host, const double *x_host);

/* ---- consumers of the path, device resident (cg.h of the reference) -------------------- */
/* (A'A + lambda I) x = b by conjugate gradients; A and the handle of its transpose as the reference passes
 * them (bsbm_cg cg.h:25); x, b: F = ncol(A) doubles in HBM; stops at ||r|| <= tol ||b|| or after F iterations.
 * Every solver below (fs_cg, fs_cg2, fs_pcg, fs_mscg, fs_pcgn, fs_pcgn_lambdas, fs_mscgn) looks at its two products before it writes anything: where one of
 * them would read plain CSR arrays that fs_matrix_release_csr gave back ("strict_order", spmv_kernel 1 / 2 / 3, the row kernel of
 * a k-column product) the solve returns FS_ERR_RELEASED with x untouched -- also a solve that would have needed no product. */
int fs_cg(fs_matrix_t A, fs_matrix_t At, double *x, const double *b, double lambda, double tol, int *out_iter,
          fs_stream_t stream);
/* the same for two right-hand sides, X and B row-major F x 2 (bsbm_cg2 cg.h:85) */
int fs_cg2(fs_matrix_t A, fs_matrix_t At, double *X, const double *B, double lambda, double tol, int *out_iter,
           fs_stream_t stream);
/* y += a x on device vectors (the "+ lambda x" of bsbm_AtA, cg.h:17-21) */
int fs_axpy(int n, double a, const double *x, double *y, fs_stream_t stream);

/* ---- preconditioned solve (no counterpart in the reference: bsbm_cg is unpreconditioned, starts from 0, reports a count) ---- */
/* d[j] = lambda + sum of v^2 over row j of At (v = 1 for a pattern-only matrix): the diagonal of A'A + lambda I, column j of A
 * taken from the transpose handle the caller of fs_cg already holds -- where no (row, column) pair is stored twice.  Entries that
 * repeat a pair (fs_coo_create keeps them apart) are squared one by one: v1^2 + v2^2 where A'A has (v1 + v2)^2.  d stays positive,
 * and as a preconditioner it changes the path of a solve, not what it converges to.  d: fs_matrix_nrow(At) doubles in HBM.  Stream-ordered, no
 * allocation.  Reads the plain CSR: FS_ERR_RELEASED after fs_matrix_release_csr.  The sum has a fixed shape and repeats its bits:
 * one wave per row; lane l starts at +0.0 and adds v * v (one multiply, one add, never fused) of entries l, l + 64, ... in
 * increasing order; the 64 lanes are folded by the __shfl_xor butterfly (32, 16, ..., 1); lambda is added last. */
int fs_gram_diag(fs_matrix_t At, double lambda, double *d, fs_stream_t stream);
enum { FS_PRECOND_NONE = 0, FS_PRECOND_JACOBI = 1, FS_PRECOND_DIAG = 2 };
typedef struct fs_pcg_params {
  double tol;          /* stop at ||r|| <= tol ||b||; negative or NaN: FS_ERR_ARG */
  int max_iter;        /* <= 0: ncol(A), the reference's cap (cg.h:55) */
  int precond;         /* FS_PRECOND_* */
  int warm_start;      /* 0: start from x = 0, x's contents ignored; 1: x holds x0 */
  const double *diag;  /* FS_PRECOND_DIAG: the caller's positive diagonal, ncol doubles in HBM; else ignored */
} fs_pcg_params;
typedef struct fs_pcg_info {
  int iterations;      /* counted as bsbm_cg counts */
  int converged;
  double rnorm, bnorm; /* sqrt of the recurrence's last r.r; sqrt(b.b) */
} fs_pcg_info;
/* (A'A + lambda I) x = b by conjugate gradients with a diagonal preconditioner M = diag(d): FS_PRECOND_JACOBI takes d from
 * fs_gram_diag(At, lambda), FS_PRECOND_DIAG from the caller, FS_PRECOND_NONE has none (z is r; no such vector is read).  A, At, x, b
 * as for fs_cg; synchronous like fs_cg; info may be NULL.  Every line is one IEEE double operation per element, `red` the
 * two-stage sum of fs_cg:
 *   dinv[j] = d[j] == 0 ? 1 : 1 / d[j], once per solve
 *   cold start: x = 0, r = b;  warm start: t = A x, q = A' t, q = q + lambda x, r = b - q
 *   bb = red(b b), rr = red(r r), stop = tol sqrt(bb);  sqrt(rr) <= stop: done, 0 iterations, x as it is (b = 0: x = 0, converged,
 *   where fs_cg returns NaN -- the only place where FS_PRECOND_NONE from a cold start with max_iter <= 0 departs from fs_cg)
 *   z = r dinv, p = z, rz = red(r z)
 *   while fewer than max_iter iterations have run:
 *     t = A p, q = A' t, q = q + lambda p, alpha = rz / red(q p), x = x + alpha p, r = r - alpha q, rr = red(r r)
 *     sqrt(rr) <= stop: done;  else z = r dinv, rzn = red(r z), beta = rzn / rz, rz = rzn, ++iterations, p = z + beta p
 * The scalars live on the device and the host learns of convergence one iteration behind, as in fs_cg; a solve that is done before
 * its first iteration enqueues no product.  Per iteration the preconditioned solve moves 14 F doubles of vector traffic (dinv is
 * read twice, z is never stored), fs_cg and FS_PRECOND_NONE 12 F.  Products add in a fixed order unless option "cg_fixed_order"
 * is 0.  FS_ERR_ARG: a NULL A, At, x, b or prm; At not of the transposed shape; precond outside 0..2; FS_PRECOND_DIAG with a NULL
 * diag; tol negative or NaN.  FS_ERR_RELEASED: FS_PRECOND_JACOBI on an At whose plain CSR was released -- raised before anything is
 * written to x (FS_PRECOND_DIAG with a diagonal kept from an earlier fs_gram_diag still works on such a handle). */
int fs_pcg(fs_matrix_t A, fs_matrix_t At, double *x, const double *b, double lambda, const fs_pcg_params *prm, fs_pcg_info *info,
           fs_stream_t stream);

/* ---- a ladder of lambdas in one solve (no counterpart in the reference) ---- */
enum { FS_MSCG_MAX_SHIFTS = 16 };
/* (A'A + lambda[i] I) x_i = b for i < m by multi-shift conjugate gradients: ONE Krylov sequence, two products per iteration
 * whatever m is.  X: m vectors of F = ncol(A) doubles in HBM, x_i at X + i * ldx (ldx >= F); b: F doubles in HBM; lambda: m
 * doubles on the HOST, any order, duplicates allowed; tol, max_iter as in fs_pcg_params; info: m entries or NULL (fs_pcg_info,
 * per shift).  Cold start only, no preconditioner.  Synchronous like fs_cg.
 * The Krylov space of A'A + lambda I from b is the same for every lambda, and the residuals of all the systems stay collinear:
 * r_i = z_i r.  So CG runs on the smallest lambda (`base`) and every other system follows from scalar recurrences on z_i and two
 * vector updates per iteration (Frommer; Jegerlehner, hep-lat/9612014).  Every line is one IEEE double operation per element,
 * `red` the two-stage sum of fs_cg:
 *   host:  base = min lambda[i];  sigma_i = lambda[i] - base            (exactly 0 for the minimum and its duplicates)
 *   start: x_i = 0, r = p = b, P_i = b;  bb = red(b b), stop = tol sqrt(bb), rsq = bb
 *          z_i = zp_i = 1, live_i = 1, count_i = 0, rn_i = sqrt(bb);  aprev = 1, bprev = 0
 *          sqrt(bb) <= stop: done -- every shift converged, 0 iterations, X = 0 (b = 0 gives 0, not NaN, as in fs_pcg);
 *          no product is enqueued
 *   iteration n = 0, 1, ... while n < cap (max_iter <= 0: F):
 *     t = A p, q = A' t, q = q + base p, alpha = rsq / red(q p)                                 -- fs_cg's kernels, fs_cg's bits
 *     S1, per live shift:  u = alpha * bprev; u = u * (zp - z);  w = sigma * alpha; w = 1 + w;  v = zp * aprev; v = v * w;
 *                          den = u + v;  zn = z * zp; zn = zn * aprev; zn = zn / den;  ratio = zn / z;  a_i = alpha * ratio
 *     update:  r = r - alpha q, rr = red(r r);  every live shift: x_i = x_i + a_i P_i
 *     S2:  s = sqrt(rr);  s <= stop: done (fs_cg MODE 2), else beta = rr / rsq, rsq = rr, ++iter
 *          per live shift: rn_i = fabs(zn) * s;
 *            !(rn_i > stop) or fabs(zn) < 2^-500 or done:  live_i = 0, converged_i = (rn_i <= stop), count_i = n   (frozen: x_i
 *            is final)
 *            else: b_i = ratio * ratio; b_i = beta * b_i;  zp = z, z = zn;  count_i = n + 1
 *          aprev = alpha, bprev = beta;  no shift live any more (only a NaN gets here without `done`): done as well
 *     direction (not done):  p = r + beta p;  every live shift: P_i = z_i r + b_i P_i   (two multiplies, one add; z_i the new one)
 *   info[i] = { count_i, converged_i, rn_i, sqrt(bb) };  a shift still live at the cap: converged 0, count = cap
 * A shift with sigma_i = 0 keeps z = 1 exactly (den = aprev, zn = 1, ratio = 1, a_i = alpha, b_i = beta): its P_i is p and its x_i
 * is fs_cg's x at that lambda, bit for bit; such shifts read p and own no direction vector.  With m = 1 the solve is fs_pcg with
 * FS_PRECOND_NONE from a cold start, info included.  Freezing is required, not an optimisation: z of a large shift underflows to
 * 0, and the next zn would be 0 / 0; the 2^-500 guard covers tol = 0, which is legal when the cap ends the solve.  A frozen shift
 * costs no traffic: per iteration with L live shifts of sigma != 0 the vector kernels move (12 + 5 L) F doubles, fs_cg 12 F,
 * plus F for every further group of four such shifts (the direction kernel reads r once per group): 3 F more at L = 15.
 * Work space per solve: 3 F + N doubles and one direction of F per shift with sigma != 0.
 * No preconditioner: a diagonal M does not commute with the shift (M^-1 (K + sigma I) is not M^-1 K + sigma I), so the
 * preconditioned Krylov spaces differ per lambda and one sequence cannot serve them.  No warm start: from x0 != 0 the residuals
 * b - (K + sigma_i I) x0 are no longer collinear, which the recurrences rest on.
 * The scalars live on the device and the host learns of convergence one iteration behind, as in fs_cg.  Products add in a fixed
 * order unless option "cg_fixed_order" is 0.  FS_ERR_ARG, raised before anything is written to X: a NULL A, At, X, b or lambda; At
 * not of the transposed shape; m outside 1..FS_MSCG_MAX_SHIFTS; ldx < F; tol negative or NaN; a lambda that is NaN or infinite.  A
 * product's own error is passed through; FS_ERR_RELEASED under "strict_order" after fs_matrix_release_csr is raised before anything
 * is written to X (see fs_cg). */
int fs_mscg(fs_matrix_t A, fs_matrix_t At, double *X, int64_t ldx, const double *b, int m, const double *lambda,
            double tol, int max_iter, fs_pcg_info *info, fs_stream_t stream);

/* ---- k right-hand sides per solve (no counterpart in the reference) ---- */
enum { FS_PCGN_MAX_RHS = 32 };
/* (A'A + lambda I) X = B for k right-hand sides on the same A (the latent dimensions of a sample, 8 to 32 of them): k INDEPENDENT
 * fs_pcg recurrences that share only the products, which run over all k columns at once (fs_spmm; k = 1: fs_spmv).  This is not
 * block CG: no shared Krylov space, no k x k solve, no breakdown when columns are dependent.  X, B: row-major F x k panels in HBM,
 * F = ncol(A), the layout of fs_spmm and fs_cg2, 8-byte aligned (16-byte aligned panels of an even k are read and written 16 bytes
 * at a time); one lambda and one prm (fs_pcg_params, as for fs_pcg: tol, max_iter, precond, warm_start -- X holds X0 --, diag) for
 * all columns, one dinv, as the matrix is the same; info: k entries or NULL.  Synchronous like fs_pcg.
 * Column j follows fs_pcg's arithmetic line by line with scalars of its own; every line is one IEEE double operation per element,
 * `red_j` the two-stage sum of fs_cg over column j's F terms -- stage 1: 1024 x 256 threads, thread (b, t) adds rows b * 256 + t,
 * + 262144, ... to +0.0 in increasing order, one multiply and one add per term, never fused, then the wave butterfly, then the four
 * waves in order; stage 2: one workgroup over the 1024 partials:
 *   dinv[i] = d[i] == 0 ? 1 : 1 / d[i], once per solve
 *   cold start: X = 0, R = B;  warm start: T = A X, Q = A' T (one pair of k-column products), Q = Q + lambda X, R = B - Q
 *   per column: bb_j = red_j(b b), rr_j = red_j(r r), stop_j = tol sqrt(bb_j), count_j = 0;
 *               sqrt(rr_j) <= stop_j: column j is frozen from the start, converged_j = 1 (b_j = 0: x_j = 0, as in fs_pcg)
 *   Z = R dinv, P = Z (every column, so that P is finite where it rides along);  live columns: rz_j = red_j(r z)
 *   every column frozen: done, no product is enqueued
 *   while fewer than max_iter iterations have run and a column is live:
 *     T = A P, Q = A' T over all k columns;  live columns: q = q + lambda p, alpha_j = rz_j / red_j(q p),
 *       x = x + alpha_j p, r = r - alpha_j q, rr_j = red_j(r r)
 *       sqrt(rr_j) <= stop_j: column j freezes, converged_j = 1
 *       else z = r dinv, rzn = red_j(r z), beta_j = rzn / rz_j, rz_j = rzn, ++count_j, p = z + beta_j p
 *   info[j] = { count_j, converged_j, sqrt(rr_j), sqrt(bb_j) };  a column still live at the cap: converged 0, count = the cap
 * Without a preconditioner z is r, r.z is r.r and no second sum runs, as in fs_pcg.  So column j is fs_pcg on B[:, j] wherever the
 * k-column product has the single-vector product's bits: bit for bit under "strict_order", and for k = 1 in every mode.
 * Freezing: once a column is frozen no kernel writes its column of X, R or P again; count_j and converged_j are final; its column
 * of P stays as it is and keeps riding through the products (wasted work of a fixed shape, unless option "pcgn_compact" moves the
 * live columns into a narrower product: "Narrowing" below).  In a row-major panel a frozen column shares its cache lines with live
 * ones, so freezing saves stores and arithmetic, not lines.  The vector kernels of an iteration come in two forms with the same bits (option "pcgn_kernel"): a lane per
 * row (k <= 4), which stops loading a cache line's worth of neighbouring columns (16 j .. 16 j + 15) once ALL of them are frozen,
 * and, for k > 4, the workgroup's 256-row panels staged through LDS with coalesced accesses, which load every line.  A column
 * whose numbers go NaN runs to the cap and changes nothing in the other columns (the products and the sums are per column).
 * The scalars live on the device (one thread per column in the one-workgroup step that finishes the sums) and the host learns of
 * `done` -- no column live -- one iteration behind, as in fs_cg.  Per iteration the vector kernels move 12 k F doubles, 14 k F
 * with a preconditioner (the formula of fs_pcg; dinv itself is read once per row, not per column).  Products add in a fixed order
 * unless option "cg_fixed_order" is 0.  Work space per solve: 3 k F + k N doubles, F more with a preconditioner, 2048 k for the
 * partial sums and 512 for the per-column scalars.
 * One-time work: for k >= 2 fs_matrix_prepare(A, k, 0) and fs_matrix_prepare(At, k, 0) run before the first iteration; their
 * errors (FS_ERR_RELEASED for a k never prepared before fs_matrix_release_csr) are raised before anything is written to X, as is
 * FS_ERR_RELEASED for FS_PRECOND_JACOBI on an At whose plain CSR was released.  FS_ERR_ARG, raised before anything is written: a
 * NULL A, At, X, B or prm; At not of the transposed shape; k outside 1..FS_PCGN_MAX_RHS; precond outside 0..2; FS_PRECOND_DIAG
 * with a NULL diag; tol negative or NaN.  A product's own error is passed through.
 * Narrowing (option "pcgn_compact" = 1; fs_pcgn and fs_pcgn_lambdas, not the sharded solvers): the solve runs in segments of
 * non-increasing width.  W(L) is the smallest of {1, 2, 4, 8, 16, 32} that is at least L: the widths at which the k-column products
 * change price.  The solve starts at width k on all k columns in the caller's X, as without the option.  m_n is the set of live
 * columns the host knows when it enqueues iteration n = 0, 1, ...: m_0 is the set after the start (the one synchronous look a
 * solve takes before its first product), m_1 = m_0, and for n >= 2 m_n is the set after iteration n - 2 (the host reads the
 * flags one iteration behind).  Before it enqueues iteration n at width w, the solve looks for the narrowest usable width w' with
 * W(|m_n|) <= w' < w; if there is one, the columns of m_n, in increasing original order, move into panels of w' columns (X, R, P;
 * Q and the products' T are overwritten anyway), followed by padding columns whose X, R, P are +0.0 and which are frozen, and
 * iteration n and those behind it run at width w' on these panels, with fs_pcgn's own kernels at k = w' (fs_pcgn_lambdas with
 * the lambdas of those columns; dinv and s are per row and stay).  Otherwise nothing moves: columns that froze without crossing a
 * width ride along as without the option.  A column that froze after the host's look travels along frozen; its scalars and its
 * live flag move with it.  A column that is left behind is final: its x goes back into the caller's X then, the last panel's
 * columns at the end, so a column of X is only ever written with values of its own recurrence, and at the return X, every info
 * and the debug getters read in original numbering as without the option.  A repack that was enqueued together with an iteration
 * which turns out not to exist (the solve was done one iteration earlier: the host learns it one behind) does nothing on the
 * device, like that iteration's other kernels, and is no segment.  At most five repacks per solve.
 * Usable widths are settled before anything is written to X: for every w < k of 16, 8, 4, 2 fs_matrix_prepare(A, w, 0) and
 * fs_matrix_prepare(At, w, 0), then the look at the two products described above fs_cg, for width 1 too; a width that answers
 * FS_ERR_RELEASED is left out, silently, and the solve is still FS_OK; any other error is returned with X untouched.
 * Work space with the option: 3 w1 F + w2 F doubles more, w1 > w2 the two widest usable widths below k (so at most 3.5 w1 F with
 * w1 the largest power of two below k: panels of X, R, P at w1 and one of X at w2; the second and fourth repack reuse the
 * full-width r and p, Q and T stay where they are), and 512 doubles for the scalars in original numbering; all of it is allocated
 * before the first iteration.  One launch per repack streams 3 (w + w') F doubles; one more, of one workgroup, moves the scalars.
 * Bits: the vector kernels and red_j give a column the same bits at every k, so wherever a w-column product has the k-column
 * product's bits -- under "strict_order", where every width runs the row kernel in storage order -- X, every info and every
 * per-column scalar are bit for bit those of option 0.  In the other modes a w-column product need not have the k-column
 * product's last bits and counts may move by rounding; the schedule depends on the counts alone, which repeat under fixed-order
 * products, so a solve with the option repeats its own bits. */
int fs_pcgn(fs_matrix_t A, fs_matrix_t At, double *X, const double *B, int k, double lambda, const fs_pcg_params *prm,
            fs_pcg_info *info /* k entries or NULL */, fs_stream_t stream);

/* (A'A + lambda[j] I) x_j = b_j for j < k: fs_pcgn with a lambda per column -- a ladder of lambdas on one b (B = b in every column),
 * or targets x rungs -- where fs_mscg cannot serve because the data need a preconditioner.  lambda: k doubles on the HOST.  All of
 * fs_pcgn's text holds (panels, alignment, prm, freezing and the live mask, option "pcgn_kernel", the one-time fs_matrix_prepare,
 * synchronous, work space, traffic: the per-column diagonal adds arithmetic, not bytes) but for what follows.
 * Arithmetic: column j follows fs_pcg at lambda[j] line by line: the warm start has Q = Q + lambda_j X, the iteration
 * q = q + lambda_j p.  FS_PRECOND_JACOBI: column j's diagonal is fs_gram_diag(At, lambda[j]), formed as s + lambda_j from ONE
 * s = fs_gram_diag(At, 0.0) per solve (the same bits: fs_gram_diag adds lambda last, and a sum of squares is never -0.0); there is
 * no pass that inverts it: the work vector holds s, and wherever fs_pcgn multiplies by dinv[i] the kernels multiply by
 *   dinv_j[i] = (s[i] + lambda_j) == 0 ? 1 : 1 / (s[i] + lambda_j)      (one IEEE addition, one IEEE division per element)
 * FS_PRECOND_DIAG: one diagonal from the caller for all columns (a caller's M need not depend on lambda), inverted once per solve
 * as in fs_pcgn.  FS_PRECOND_NONE: no diagonal is read.
 * So column j IS fs_pcg at lambda[j] on B[:, j] wherever the k-column product has the single-vector product's bits: bit for bit
 * under "strict_order", and for k = 1 in every mode.  With all lambda[j] equal the solve is fs_pcgn at that lambda, bit for bit,
 * in every mode in which fs_pcgn repeats its own bits.
 * FS_ERR_ARG, raised before anything is written to X: what fs_pcgn refuses; a NULL lambda; a lambda that is NaN or infinite.
 * FS_ERR_RELEASED as in fs_pcgn. */
int fs_pcgn_lambdas(fs_matrix_t A, fs_matrix_t At, double *X, const double *B, int k,
                    const double *lambda /* k doubles on the HOST */, const fs_pcg_params *prm,
                    fs_pcg_info *info /* k entries or NULL */, fs_stream_t stream);

/* (A'A + lambda[i] I) x_ij = b_j for i < m, j < k: a ladder of m lambdas, shared by all targets, for k right-hand sides in one solve
 * -- targets x rungs on data that need no preconditioner -- on ONE pair of k-column products per iteration, where fs_pcgn_lambdas
 * runs k m columns through the products.  Not block CG: column j is fs_mscg on B[:, j], line by line, with scalars of its own; the
 * columns share only the products.  fs_mscg's text is the single statement of the shift recurrences; this says what differs.
 * B: a row-major F x k panel in HBM, F = ncol(A), with the layout and alignment rules of fs_pcgn.  X: m such panels, the panel of
 * lambda[i] at X + i * ldx, ldx >= F * k; doubles in the gaps are never touched.  A panel is accessed 16 bytes at a time only where
 * k is even and that panel's address is 16-byte aligned; the results do not depend on this.  k in 1..FS_PCGN_MAX_RHS, m in
 * 1..FS_MSCG_MAX_SHIFTS; lambda: m doubles on the HOST, any order, duplicates allowed; tol, max_iter as in fs_mscg; info: m * k
 * entries, info[i * k + j], or NULL.  Cold start only, no preconditioner, for fs_mscg's reasons.  Synchronous like fs_mscg.  Option
 * "pcgn_compact" is not read.
 * Arithmetic.  The host forms base and the sigma_i once, for every column.  Per column j: bb_j, stop_j, rsq_j, alpha_j, beta_j,
 * aprev_j, bprev_j and the iteration count; per pair (i, j): z, zp, zn, ratio, a, b, rn, live, converged, count -- fs_mscg's per-shift
 * scalars.  `red_j` is fs_pcgn's: fs_cg's two-stage tree over column j's F terms.
 *   start: X_i = 0 for all i, R = P = B, P_i = B for every shift with sigma_i != 0;  bb_j = red_j(b b), fs_mscg's start per column.
 *          sqrt(bb_j) <= stop_j (b_j = 0; tol >= 1): column j is frozen from the start, all its pairs converged with count 0 and
 *          x_ij = +0.0.  Every column frozen: done, no product is enqueued
 *   iteration n = 0, 1, ... while n < cap (max_iter <= 0: F) and a column is live, over live columns and live pairs only:
 *     T = A P, Q = A' T: one pair of k-column products (fs_spmm; k = 1: fs_spmv)
 *     q_j = q_j + base p_j, alpha_j = rsq_j / red_j(q p)                                 -- fs_pcgn's kernels at lambda = base
 *     S1 of fs_mscg for every live pair, with column j's alpha, aprev, bprev
 *     r_j = r_j - alpha_j q_j, rr_j = red_j(r r)                                         -- fs_pcgn's kernel, X left alone
 *     x_ij = x_ij + a_ij P_ij for every live pair (a pair with sigma_i = 0 reads column j of P)
 *     S2 of fs_mscg per column, `done` being sqrt(rr_j) <= stop_j: a column that is done freezes, and with it every pair it still
 *       has; so does a column that has no live pair left (only when a NaN froze them all: fs_mscg's freeze rule
 *       !(rn > stop) or fabs(zn) < 2^-500 or done holds per pair, and a NaN fails rn > stop)
 *     direction: p_j = r_j + beta_j p_j for the live columns;  P_ij = z_ij r_j + b_ij P_ij for the live pairs (two multiplies, one
 *       add; z the new one)
 *   info[i * k + j] = { count_ij, converged_ij, rn_ij, sqrt(bb_j) };  a pair still live at the cap: converged 0, count = cap
 * So column j of panel i is fs_mscg's x_i on B[:, j] wherever the k-column product has the single-vector product's bits: bit for
 * bit under "strict_order", and for k = 1 in every mode.  With m = 1 the solve is fs_pcgn with FS_PRECOND_NONE from a cold start at
 * lambda[0], bit for bit, infos included, in every mode in which fs_pcgn repeats its own bits.  Pairs of the smallest lambda and its
 * duplicates keep z = 1 exactly and own no direction panel.
 * Freezing: no kernel changes a frozen pair's x_ij or P_ij again; a frozen column's columns of R and P keep their bits, and its P
 * rides through the products as in fs_pcgn.  A shift none of whose pairs is live costs no traffic: its panels X_i and P_i are not
 * read.  In a row-major panel a frozen pair shares its cache lines with live ones, so it saves stores and arithmetic, not lines.  A
 * column whose numbers go NaN changes no bit of another column (the products and the sums are per column); its pairs freeze
 * unconverged by fs_mscg's rule, at the count fs_mscg reports for that column.
 * The scalars live on the device; the host learns of `done` -- no column live -- one iteration behind, as in fs_cg.  Products add in
 * a fixed order unless option "cg_fixed_order" is 0; option "pcgn_kernel" picks the form of the two kernels that take sums.
 * Traffic: the kernels that take sums move 6 k F doubles per iteration whatever is frozen (q + base p: 3, r - alpha q: 3).  The
 * pair kernels stream whole panels flat: per shift that still has a live pair 3 k F for x (P_i or P, x_i in, x_i out) and, with
 * sigma_i != 0, 2 k F for P_i; the direction pass moves 3 k F for P itself and reads R once more per further group of four shifts.
 * With one sigma = 0 shift and L others live that is (12 + 5 L) k F, fs_mscg's formula per column, plus k F per further group of four
 * and 3 k F per duplicate of the smallest lambda.  k = 8, L = 7, F = 10 M: 30 GB per iteration.
 * Work space per solve: 3 k F + k N doubles (R, P, Q, T), one F x k direction panel per shift with sigma != 0, 2048 k doubles for
 * the partial sums and 9344 for the scalars; all of it is allocated before the first store to X.  Mind the size: k = 8, m = 16,
 * F = 10 M is 10 GB of X and 9.6 GB of directions.
 * One-time work: for k >= 2 fs_matrix_prepare(A, k, 0) and fs_matrix_prepare(At, k, 0) run first, then the look at the two products
 * described above fs_cg.  FS_ERR_ARG, raised before anything is written to X: a NULL A, At, X, B or lambda; At not of the transposed
 * shape; k outside 1..FS_PCGN_MAX_RHS; m outside 1..FS_MSCG_MAX_SHIFTS; ldx < F * k; tol negative or NaN; a lambda that is NaN or
 * infinite.  FS_ERR_RELEASED, with X untouched: under "strict_order" after fs_matrix_release_csr; for a k never prepared before the
 * release.  A failed allocation of the work space returns FS_ERR_HIP with X untouched.  A product's own error is passed through. */
int fs_mscgn(fs_matrix_t A, fs_matrix_t At, double *X, int64_t ldx, const double *B, int k, int m,
             const double *lambda /* m doubles on the HOST */, double tol, int max_iter,
             fs_pcg_info *info /* m * k entries, info[i * k + j], or NULL */, fs_stream_t stream);

/* ---- column-blocked binary CSR (cbcsr.h) -------------------------------------------- */
fs_cbcsr_t fs_cbcsr_create(int nrow, int ncol, int nblocks, int colblocksize, const int *row_ptr,
                           const int *cols, int space);
void fs_cbcsr_destroy(fs_cbcsr_t A);
/* y[nrow] = A x: per column block the x tile is staged in LDS, cell sums are added block by block */
int fs_cbcsr_spmv(fs_cbcsr_t A, double *y, const double *x, fs_stream_t stream);

/* ---- several GPUs, one process (fs_dist.hip) ------------------------------------------------
 * Rows are cut into one contiguous shard per device with (almost) equal numbers of non-zeros, every device holds the
 * whole x, multiplies its shard with the single-GPU kernels and the y shards are all-gathered over RCCL (xGMI), so that
 * every device ends up with the whole y: the reference's row-parallel `omp parallel for` (csr.h:429) across devices
 * (SURVEY.md 8e).  The exchange runs INSIDE the product: the local product is cut into FS_DIST_PARTS parts (default 4,
 * fs_spmv_part) and the ncclAllGather of the rows a part finished -- one call per part on a padded buffer, the ranks' calls
 * in one group -- runs on a second stream under the later parts; one fs_copy_segments launch unpacks.  z = A' u is the same
 * scheme on row shards of A' (fs_dist_matrix_build_transpose), with u = the y of the last product in place.
 * librccl.so is loaded with dlopen when a context with more than one distinct device is created.
 * A C caller of ANY product entry point of sparse.h / dsparse.h / csr.h / cbcsr.h / cg.h gets this path by setting
 * FASTSPARSE_NGPU=N (optionally FASTSPARSE_DEVICES=0,1,...) in the environment (fs_dropin.hip, "several GPUs").
 * devices == NULL means devices 0 .. ndev-1; ndev < 1 means every visible device.  A device may be listed more than once
 * ("virtual ranks" on one GPU, for testing the sharding on a one-GPU machine): such a context exchanges the parts
 * with device-to-device copies, because RCCL refuses duplicate devices.  Products on one fs_dist_matrix_t are serialised
 * by a lock (its vectors and part buffers are per matrix). */
fs_dist_t fs_dist_create(int ndev, const int *devices);
void fs_dist_destroy(fs_dist_t D);
int  fs_dist_ndev(fs_dist_t D);
int  fs_dist_uses_rccl(fs_dist_t D);
/* 1 once the context exchanges conservatively: ONE whole-shard all-gather behind the finished local product instead of one per
 * part under the later parts.  Chosen with FS_DIST_PARTS=1, and taken for good when a group call of the overlapped mode returns an
 * error on VIRTUAL ranks (that product is finished conservatively).  With RCCL a failed group call aborts the communicators
 * (ncclCommAbort): that product and every later one on the context return the error -- no second collective is attempted on a
 * half-issued group.  The overlapped mode is UNVERIFIED on more than one GPU. */
int  fs_dist_is_conservative(fs_dist_t D);
/* host CSR arrays -> nnz-balanced row shards, one fs_matrix_t per device; vals == NULL: pattern-only */
fs_dist_matrix_t fs_dist_csr_create(fs_dist_t D, int nrow, int ncol, int64_t nnz, const int *row_ptr, const int *cols,
                                    const double *vals);
/* host COO arrays (vals == NULL: pattern-only) -> the same shards; the entries are bucketed stably by row first (new_csr / new_bcsr,
 * csr.h:375-422, 30-67), so every row adds in the caller's entry order like the serial COO loops (sparse.h:58-65, dsparse.h:43-51):
 * A_mul_B / sdm_A_mul_B / bsbm_* / bsdm_* across the GPUs.  At_mul_B passes (cols, rows). */
fs_dist_matrix_t fs_dist_coo_create(fs_dist_t D, int nrow, int ncol, int64_t nnz, const int *rows, const int *cols, const double *vals);
/* A and its transpose as the caller holds them -- TWO matrices, like bsbm_cg(x, B, Bt, ...) cg.h:25 -- as one handle for fs_dist_cg /
 * fs_dist_cg2 / fs_dist_ata / the *_t products: direct side = A's, transposed side = At's direct side (a row of A' adds in the order
 * the caller's own At stores it).  Shares the shards of both (no copy; they live until the last of the three handles is destroyed, in
 * any order); own vectors and solver work space.  The cuts of its transposed side are At's row cuts, whatever the caller chose
 * (fs_dist_matrix_bounds_t; empty shards anywhere, one-row shards): scheme 1 of fs_dist_cg / fs_dist_pcg slices by them.  It HAS its
 * transposed side: fs_dist_matrix_build_transpose[_device] on a pair return FS_OK and build nothing.  NULL with a message in
 * fs_last_error(): a NULL handle, handles of two contexts, shapes that are not each other's transposes.  The single-vector exchange
 * buffers belong to a side, so to every handle that shares it: products on different handles of one context are ordered by the
 * context's lock. */
fs_dist_matrix_t fs_dist_matrix_pair(fs_dist_matrix_t A, fs_dist_matrix_t At);
/* The matrix as per-rank shards -- no whole-matrix array anywhere, so the TOTAL may exceed 2^31 - 1 entries (every shard stays
 * below it: int row_ptr, csr.h:358-366); BASELINE config 5 (3.2 G entries, 8 shards) enters this way.  Shard r = the next
 * shard_rows[r] rows of A: a LOCAL row_ptr (shard_rows[r] + 1 ints from 0), GLOBAL column ids, optional values (vals == NULL or
 * vals[r] == NULL for all r: pattern-only).  space = FS_HOST: host arrays; FS_DEVICE: shard r's arrays are on rank r's device
 * (copied; the caller may free them).  The caller chooses the cuts (by non-zeros for power-law matrices). */
fs_dist_matrix_t fs_dist_csr_create_from_shards(fs_dist_t D, int nrow, int ncol, const int *shard_rows /* ndev */,
                                                const int64_t *shard_nnz /* ndev */, const int *const *row_ptr, const int *const *cols,
                                                const double *const *vals, int space);
void fs_dist_matrix_destroy(fs_dist_matrix_t M);
/* row shards of A' (columns of A cut by non-zeros; every row of A' in ascending A-row order) from the SAME host arrays the
 * matrix was created from (the handle keeps no host copy); idempotent */
int  fs_dist_matrix_build_transpose(fs_dist_matrix_t M, const int *row_ptr, const int *cols, const double *vals);
/* the same shards of A' from the device-resident shards of A: per-rank column counts added up and cut on one device, a stable
 * partition of every shard's entries by owner, device-to-device copies, a stable local sort -- no host array of the matrix
 * (what a matrix created from shards needs; works for any).  Same bounds, same entry order as the host build.  Idempotent. */
int  fs_dist_matrix_build_transpose_device(fs_dist_matrix_t M);
int  fs_dist_matrix_has_transpose(fs_dist_matrix_t M);
int  fs_dist_matrix_bounds(fs_dist_matrix_t M, int *bounds /* ndev + 1: row cuts of A */);
int  fs_dist_matrix_bounds_t(fs_dist_matrix_t M, int *bounds /* ndev + 1: row cuts of A' = column cuts of A */);
int64_t fs_dist_matrix_shard_nnz(fs_dist_matrix_t M, int rank);
int64_t fs_dist_matrix_nnz(fs_dist_matrix_t M);
/* the handle of rank `rank`'s shard of A (transposed != 0: of A'), owned by M, on that rank's device: for inspection
 * (fs_matrix_download, fs_matrix_spmv_kernel, fs_matrix_device_bytes) */
fs_matrix_t fs_dist_matrix_shard(fs_dist_matrix_t M, int rank, int transposed);
/* y[nrow] = A x[ncol] / z[ncol] = A' u[nrow]; synchronous.  The vectors may be in HOST memory -- the input goes to every device over
 * its own PCIe link through a pinned staging buffer (chunks, the host copy of the next under the uploads of the last), the output
 * comes back from device 0 -- or in HBM of any device (hipPointerGetAttributes decides, per vector): then nothing touches the host.
 * The ranks on the input's device read it in place, the others receive it device to device; an output in HBM IS the gathered vector
 * of the first rank on its device (the unpack launch writes it).  The caller's earlier work on the legacy default stream of those
 * devices is waited for first.  The same holds for every fs_dist_* function below that takes vectors. */
int  fs_dist_spmv(fs_dist_matrix_t M, double *y, const double *x);
int  fs_dist_spmv_t(fs_dist_matrix_t M, double *z, const double *u);
/* z[ncol] = A'(A x[ncol]) + lambda x: bcsr_AA_mul_B / parallel_bcsr_AA_mul_B (csr.h:305-355; lambda = 0) and bsbm_AtA (cg.h:9-22)
 * across the GPUs; A x stays on the devices */
int  fs_dist_ata(fs_dist_matrix_t M, double *z, const double *x, double lambda);
/* device-resident forms for iterating callers: fill fs_dist_x(M, r) (ncol doubles on rank r's device) on every rank ONCE;
 * fs_dist_spmv_resident leaves y = A x in fs_dist_y(M, r) (nrow doubles, complete on every rank when the call returns),
 * fs_dist_spmv_t_resident leaves z = A' y in fs_dist_z(M, r) (y of the last product is u, in place), fs_dist_swap_xy makes y
 * the next x (square matrices: power iteration) -- nothing crosses PCIe between products */
int  fs_dist_spmv_resident(fs_dist_matrix_t M);
int  fs_dist_spmv_t_resident(fs_dist_matrix_t M);
int  fs_dist_swap_xy(fs_dist_matrix_t M);
/* (A'A + lambda I) x = b by conjugate gradients on the sharded matrix (bsbm_cg, cg.h:25-82, across the GPUs): everything
 * resident, the scalars of the iteration on the devices.  Option "dist_cg_scheme" 0: the vector steps replicated on every
 * device (identical vectors everywhere, the dots need no exchange, both products carry their all-gather); 1: every device keeps
 * its slice of the unknowns (vector work divided by the devices; the partial dots are all-gathered, 8 bytes per rank, and added in
 * rank order; the new search direction is all-gathered).  Every device decides convergence for itself and the host compares
 * the flags of all of them: a disagreement is an error return (FS_ERR_HIP), not a hang.  Products add in a fixed order unless
 * option "cg_fixed_order" is 0.  b_host, x_host: ncol doubles; stops at ||r|| <= tol ||b||.
 * CLOBBERS fs_dist_x / fs_dist_y / fs_dist_z (they are the solver's work vectors): upload x again before the next resident product. */
int  fs_dist_cg(fs_dist_matrix_t M, double *x_host, const double *b_host, double lambda, double tol, int *out_iter);
/* The preconditioned solvers on the sharded matrix.  Their arithmetic is that of fs_gram_diag / fs_pcg / fs_pcgn above, whose text
 * is the single statement of it; what follows says only what differs.  All three need the transposed side (FS_ERR_NO_TRANSPOSE; it
 * may come from fs_dist_matrix_build_transpose, _device or fs_dist_matrix_pair), are synchronous like fs_dist_cg, and take their
 * vectors (x, b, d, prm->diag, the row-major ncol x k panels X, B) in host memory or in HBM of any device, like fs_dist_spmv:
 * nothing in HBM is staged through the host.  The caller's x / X is written once, at the end of a solve that succeeded.
 *
 * fs_dist_gram_diag: d[ncol] = fs_gram_diag of A'.  Rank r runs it over the rows of A' it owns; one whole-shard all-gather gives
 * every rank the whole d.  A row of A' lives on one rank, so the bits are fs_gram_diag's on the same A', for any number of ranks,
 * in every mode.  FS_ERR_ARG: a NULL M or d.  FS_ERR_RELEASED: a rank's shard of A' gave its plain CSR back (fs_matrix_release_csr
 * on a fs_dist_matrix_shard handle) -- raised before anything is written.  CLOBBERS fs_dist_z. */
int  fs_dist_gram_diag(fs_dist_matrix_t M, double lambda, double *d /* ncol */);
/* fs_dist_pcg: fs_pcg with fs_pcg_params / fs_pcg_info unchanged (tol, max_iter, precond, warm_start -- x holds x0 --, diag).
 * Option "dist_cg_scheme" as for fs_dist_cg:
 *   0  every rank holds whole x, r, p, q, dinv and launches fs_pcg's own kernels on them: identical kernels on identical data, no
 *      exchange for the sums.  `red` is fs_pcg's: under "strict_order" x, fs_pcg_info and the scalars are fs_pcg's on the same CSRs,
 *      bit for bit, for any number of ranks.  FS_PRECOND_JACOBI costs the one all-gather of d per solve, a warm start one pair of
 *      sharded products on x0 in front.
 *   1  rank r keeps its slice of x, r, p, q, dinv: the rows of A' it owns.  Jacobi's slice of d is the rank's own launch: no
 *      exchange.  `red` is the slice tree of fs_dist_cg: every rank reduces its slice with fs_cg's two stages, the rank values are
 *      all-gathered and every rank adds them in rank order with the second stage (an empty slice contributes +0.0).  The sums fs_pcg
 *      takes in one pass travel in one exchange of two doubles per rank ({bb, rr} at the start; {rr, rzn} with a preconditioner),
 *      so an iteration has two small exchanges and the all-gather of the new p, like fs_dist_cg.  Every other line is fs_pcg's.
 * Either way every rank decides convergence for itself and the host compares the flags of all of them one iteration behind, as in
 * fs_dist_cg: a disagreement is an error return (FS_ERR_HIP).  A solve that is done before its first iteration enqueues no product
 * for an iteration and leaves x as fs_pcg does (b = 0: x = 0, converged, where fs_dist_cg returns NaN).  Products add in a fixed
 * order unless option "cg_fixed_order" is 0.  Work vectors stay on the handle between solves.  FS_ERR_ARG: a NULL M, x, b or prm;
 * precond outside 0..2; FS_PRECOND_DIAG with a NULL diag; tol negative or NaN.  FS_ERR_RELEASED: FS_PRECOND_JACOBI when a rank's
 * shard of A' gave its plain CSR back (FS_PRECOND_DIAG with a diagonal kept from before still solves).  Every one of them is raised
 * before anything is written to x.  CLOBBERS fs_dist_x / fs_dist_y / fs_dist_z like fs_dist_cg. */
int  fs_dist_pcg(fs_dist_matrix_t M, double *x, const double *b, double lambda, const fs_pcg_params *prm, fs_pcg_info *info /* or NULL */);
/* fs_dist_pcgn: fs_pcgn, k in 1..FS_PCGN_MAX_RHS.  Replicated on every rank WHATEVER "dist_cg_scheme" says (the slice-wise form is
 * fs_dist_pcgn_lambdas with equal lambdas): whole ncol x k panels per rank, fs_pcgn's own kernels (option "pcgn_kernel", the live mask,
 * freezing) on them, T = A P and Q = A' T as the sharded k-column products of fs_dist_spmm (k = 1: fs_dist_spmv's).  Column j is
 * fs_pcgn's column j and therefore fs_pcg on B[:, j] wherever the sharded k-column product has the single-vector product's bits
 * ("strict_order"; k = 1 in every mode).  Convergence across the ranks, a solve done before its first iteration, the fixed order of
 * the products, the work space and the clobbered vectors as for fs_dist_pcg (the k-column vectors of fs_dist_spmm for k > 1).
 * FS_ERR_ARG: those of fs_dist_pcg (X, B for x, b) and k out of range; FS_ERR_RELEASED as there; raised before anything is written
 * to X.
 * Option "pcgn_compact" is not read here nor by fs_dist_pcgn_lambdas: the sharded solves run every iteration on all k columns. */
int  fs_dist_pcgn(fs_dist_matrix_t M, double *X, const double *B, int k, double lambda, const fs_pcg_params *prm,
                  fs_pcg_info *info /* k entries or NULL */);
/* fs_dist_pcgn_lambdas: fs_pcgn_lambdas on the sharded matrix -- (A'A + lambda[j] I) x_j = b_j for j < k, k in
 * 1..FS_PCGN_MAX_RHS.  Its arithmetic is fs_pcgn_lambdas' above, whose text is the single statement of it; this says only what
 * differs.  X, B, the transposed side, the statuses, a solve done at its start, the work space kept on the handle and the clobbered
 * vectors are fs_dist_pcgn's; lambda: k doubles on the host, a NULL, NaN or infinite one is FS_ERR_ARG.  Unlike fs_dist_pcgn it
 * honours option "dist_cg_scheme"; slices only with more than one rank:
 *   0  fs_dist_pcgn's frame with fs_pcgn_lambdas' instantiations of the kernels on whole panels.  Under FS_PRECOND_JACOBI the work
 *      vector holds s = fs_gram_diag of A' at 0.0, all-gathered once; there is no inverse pass.  `red_j` is fs_pcgn's: under
 *      "strict_order" X, the infos, st[] and the per-column scalars are fs_pcgn_lambdas' on the same CSRs, bit for bit, for any number
 *      of ranks; with equal lambdas the solve is fs_dist_pcgn, bit for bit.
 *   1  rank r keeps its rows [lo_r, hi_r) = fs_dist_matrix_bounds_t of X, R, B, Q and of s / dinv: contiguous (hi_r - lo_r) k
 *      doubles of the row-major panels.  P and T = A P stay whole on every rank (the product's input and output); the rank's slice
 *      of P lives in the exchange's own send buffer.  T = A P is one sharded k-column product with its all-gather, Q_r = A'_r T the
 *      rank's own shard product (fs_spmm on fs_dist_matrix_shard(M, r, 1); fs_spmv for k = 1): no exchange.  Jacobi's slice of s is
 *      the rank's own fs_gram_diag launch.  `red_j` is the slice tree of fs_dist_cg, per column: every rank reduces its slice with
 *      fs_cg's two stages (row indices local to the slice, an empty slice gives +0.0), the rank values are all-gathered and every
 *      rank adds them in rank order with the second stage.  The sums fs_pcgn takes in one pass travel in one exchange of ns k
 *      doubles per rank ({bb_j, rr_j} at the start, {rr_j, rzn_j} with a preconditioner, one sum otherwise; a frozen column's slots
 *      are sent as +0.0 and never read), so an iteration has two small exchanges and the all-gather of the new P slices, like
 *      fs_dist_pcg.  The first P is Z = R dinv, which only the owner of a row can form: it is gathered too, also on a cold start.
 *      Every rank runs the per-column scalar step over the same gathered values, so alpha_j, beta_j, the freezes and the live mask
 *      are identical everywhere.  A warm start takes the whole X0 as the product's input plus the rank's slice; T = A X0 is one
 *      sharded product, Q_r = A'_r T local.  Every other line is fs_pcgn_lambdas'.  Work space per rank: five slices of n_r k
 *      doubles (X, R, B, Q, and P in the send buffer), the whole P (ncol k) and T (nrow k), the slice of s / dinv, the partials,
 *      two send slots of 2 FS_PCGN_MAX_RHS doubles and N times that for the gathered values.
 * Besides {done, iterations}, compared one iteration behind, every rank's final live mask and per-column {live, converged, count}
 * must agree with rank 0's: a disagreement is an error return (FS_ERR_HIP).  A solve that is done at its start enqueues no product
 * and freezes every column at its start as fs_pcgn does (b_j = 0: x_j = 0; a warm column keeps x0_j).  A product's own error is
 * passed through with X untouched.  fs_debug_last_cg_state and fs_debug_last_pcgn_state report rank 0's. */
int  fs_dist_pcgn_lambdas(fs_dist_matrix_t M, double *X, const double *B, int k, const double *lambda /* k doubles on the HOST */,
                          const fs_pcg_params *prm, fs_pcg_info *info /* k entries or NULL */);
/* fs_dist_mscg: fs_mscg on the sharded matrix -- (A'A + lambda[i] I) x_i = b for i < m from one Krylov sequence, m in
 * 1..FS_MSCG_MAX_SHIFTS.  Its arithmetic is fs_mscg's above, whose text is the single statement of it; this says only what differs.
 * x_i at X + i * ldx (ldx >= ncol); X and b in host memory or in HBM of any device of the context, decided per vector as for
 * fs_dist_pcg: nothing in HBM is staged through the host.  lambda: m doubles on the host; info: m entries or NULL.  Needs the
 * transposed side (FS_ERR_NO_TRANSPOSE; from fs_dist_matrix_build_transpose, _device or fs_dist_matrix_pair), is synchronous, cold
 * start only and without a preconditioner, for fs_mscg's reasons.  Option "dist_cg_scheme" as for fs_dist_pcg; slices only with more
 * than one rank:
 *   0  every rank holds whole r, p, q, the m x_i and the directions P_i and launches fs_mscg's own kernels on them; both products
 *      carry their all-gather, nothing is exchanged for the sums.  `red` is fs_mscg's: under "strict_order" X, fs_pcg_info, the
 *      scalars and the per-shift array are fs_mscg's on the same CSRs, bit for bit, for any number of ranks.
 *   1  rank r keeps its slice -- the rows of A' it owns -- of r, p, q, every x_i and every P_i.  The x_i and P_i never leave their
 *      rank: only p enters a product, so an iteration costs fs_dist_cg's exchanges (two sums of 8 bytes per rank, one all-gather of
 *      p) however many shifts there are, and the (12 + 5 L) F doubles the vector kernels move are divided by the ranks, as is the
 *      (m + nslots) F work space.  q_r = A'_r y is the rank's own shard.  `red` (b b, q p, r r) is the slice tree of fs_dist_cg: the
 *      rank reduces its slice with both stages, the rank values are all-gathered and added in rank order by the second stage (an
 *      empty slice gives +0.0); start, S1 and S2 then run on every rank over the same N values, so every rank holds identical
 *      alpha, zn, a_i, b_i, freezes and list of live shifts.  The first p is b, which every rank holds whole: no gather before the
 *      first product.
 * Every rank decides convergence for itself as in fs_dist_cg; besides {done, iterations} every rank's per-shift {live, converged,
 * count} must agree with rank 0's: a disagreement is an error return (FS_ERR_HIP).  X is written ONCE, at the end of a solve that
 * succeeded: every refusal and every product error leaves all of X untouched.  A solve that is done at its start (b = 0, tol >= 1)
 * enqueues no product: X = 0, every shift converged, 0 iterations.  The x_i, the P_i and the per-shift array stay on the handle
 * between solves (re-made when a solve needs more or longer vectors, freed by fs_dist_matrix_destroy); r, b, p, q are fs_dist_pcg's.
 * FS_ERR_ARG, raised before anything else happens: a NULL M, X, b or lambda; m outside 1..FS_MSCG_MAX_SHIFTS; ldx < ncol; tol
 * negative or NaN; a lambda that is NaN or infinite.  A product's own error is passed through (FS_ERR_RELEASED under "strict_order"
 * on a shard that gave its plain CSR back).  CLOBBERS fs_dist_x / fs_dist_y / fs_dist_z like fs_dist_cg. */
int  fs_dist_mscg(fs_dist_matrix_t M, double *X, int64_t ldx, const double *b, int m, const double *lambda /* host */,
                  double tol, int max_iter, fs_pcg_info *info /* m entries or NULL */);
/* fs_dist_mscgn: fs_mscgn on the sharded matrix -- (A'A + lambda[i] I) x_ij = b_j for i < m, j < k on one pair of k-column products
 * per iteration, m in 1..FS_MSCG_MAX_SHIFTS, k in 1..FS_PCGN_MAX_RHS.  Its arithmetic is fs_mscgn's above, whose text is the single
 * statement of it; this says only what differs.  B: a row-major ncol x k panel; panel i of X at X + i * ldx (ldx >= ncol * k, the
 * gaps are never touched); X and B in host memory or in HBM of any device of the context, decided per pointer as for fs_dist_mscg:
 * nothing in HBM is staged through the host.  lambda: m doubles on the host.  Needs the transposed side (FS_ERR_NO_TRANSPOSE; from
 * fs_dist_matrix_build_transpose, _device or fs_dist_matrix_pair), is synchronous, cold start only and without a preconditioner.
 * Option "pcgn_compact" is not read.  Option "dist_cg_scheme" as for fs_dist_mscg; slices only with more than one rank:
 *   0  every rank holds whole panels R, P, Q, the m X_i and the direction panels and launches fs_mscgn's own steps on them; T = A P
 *      and Q = A' T are the sharded k-column products of fs_dist_spmm (k = 1: fs_dist_spmv's), nothing is exchanged for the sums.
 *      `red_j` is fs_mscgn's: under "strict_order" X, every info and every column's scalars and per-shift array are fs_mscgn's on
 *      the same CSRs, bit for bit, for any number of ranks.
 *   1  rank r keeps its rows [lo_r, hi_r) = fs_dist_matrix_bounds_t of R, Q, every X_i and every P_i: contiguous (hi_r - lo_r) k
 *      doubles of the row-major panels, which the flat pair kernels take as panels of fewer rows.  P and T = A P stay whole on every
 *      rank; the rank's slice of P lives in the k-column exchange's own send buffer, as in fs_dist_pcgn_lambdas.  The X_i and P_i
 *      never leave their rank: only P enters a product.  An iteration is one sharded product T = A P, the rank's own shard product
 *      Q_r = A'_r T (fs_spmm on the shard; fs_spmv for k = 1), two small exchanges of k doubles per rank (q p, then r r) and the
 *      all-gather of the new P slices, however many shifts there are; the (12 + 5 L) k F doubles the vector kernels move and the
 *      (m + nslots) k F doubles of panels are divided by the ranks.  The first P is B, which every rank holds whole after staging:
 *      no gather before the first product; the start exchanges {bb_j, rr_j}, 2 k doubles per rank.  `red_j` is the slice tree of
 *      fs_dist_cg, per column, as in fs_dist_pcgn_lambdas: the rank's partial sums are finished into its send slot (row indices
 *      local to the slice, an empty slice gives +0.0, a frozen column's slots are sent as +0.0 and never read), all-gathered and
 *      added in rank order with the second stage.  Start, S1 and S2 of fs_mscg then run per column on every rank over the same
 *      values, so alpha_j, the a_ij and b_ij, every freeze, the per-shift masks and the list of live shifts are identical everywhere.
 * Work space per rank, kept on the handle between solves (the panels re-made when a solve needs more or longer ones, all of it
 * freed by fs_dist_matrix_destroy), n_r = ncol under scheme 0 and hi_r - lo_r under scheme 1: m + nslots panels of n_r k doubles
 * (rounded up to an even count) for the X_i and the P_i; fs_dist_pcgn_lambdas' own for k columns, of which this solve uses R, B
 * (and Q under scheme 1) of n_r k doubles, 2048 k doubles of partial sums, two send slots of 2 FS_PCGN_MAX_RHS doubles and N times
 * that for the gathered values; 9344 doubles of scalars; and the whole P (ncol k), T (nrow k) and Q (ncol k) of the sharded
 * k-column products, with the slice of P in their send buffer.
 * Every rank decides convergence for itself as in fs_dist_cg; {done, iterations} is compared one iteration behind, and at the end
 * every rank's mask of live columns, every column's done flag and every pair's {live, converged, count} must agree with rank 0's: a
 * disagreement is an error return (FS_ERR_HIP).  X is written ONCE, at the end of a solve that succeeded -- scheme 0: whole panels
 * from rank 0; scheme 1: every rank stores its rows at X + i * ldx + lo_r k --: every refusal and every product error leaves all
 * of X untouched.  A solve that is done at its start (B = 0, tol >= 1) enqueues no product: X = +0.0, every pair converged, 0
 * iterations.  fs_debug_last_cg_state and fs_debug_last_mscgn_state report rank 0's.
 * FS_ERR_ARG, raised before anything else happens: a NULL M, X, B or lambda; k outside 1..FS_PCGN_MAX_RHS; m outside
 * 1..FS_MSCG_MAX_SHIFTS; ldx < ncol * k; tol negative or NaN; a lambda that is NaN or infinite.  A product's own error is passed
 * through (FS_ERR_RELEASED under "strict_order" on a shard that gave its plain CSR back).  CLOBBERS fs_dist_x / fs_dist_y /
 * fs_dist_z and the k-column vectors of fs_dist_spmm, like fs_dist_pcgn. */
int fs_dist_mscgn(fs_dist_matrix_t M, double *X, int64_t ldx, const double *B, int k, int m,
                  const double *lambda /* m doubles on the HOST */, double tol, int max_iter,
                  fs_pcg_info *info /* m * k entries, info[i * k + j], or NULL */);
/* k row-major columns across the GPUs (csr_A_mul_Bn csr.h:441, bcsr_A_mul_Bn csr.h:257, bsbm_A_mul_Bn sparse.h:318): every device
 * multiplies its shard with the k-column kernels of fs_spmm (prepared on the first call with a new k: synchronous) and the Y shards
 * are all-gathered -- inside the product, part by part, where the k-column product finishes its rows that way (the one-sweep plan
 * of k = 2, 4: fs_spmm_part), otherwise in one whole-shard exchange behind it; host matrices Y[nrow, k], X[ncol, k] / Z[ncol, k], U[nrow, k]; k = 1 is fs_dist_spmv */
int  fs_dist_spmm(fs_dist_matrix_t M, double *Y_host, const double *X_host, int k);
int  fs_dist_spmm_t(fs_dist_matrix_t M, double *Z_host, const double *U_host, int k);
/* (A'A + lambda I) X = B with two right-hand sides, row-major ncol x 2: bsbm_cg2 (cg.h:85-187) across the GPUs; the vector steps
 * and the 2x2 algebra replicated on every device, convergence compared across all devices like fs_dist_cg */
int  fs_dist_cg2(fs_dist_matrix_t M, double *X_host, const double *B_host, double lambda, double tol, int *out_iter);
double *fs_dist_x(fs_dist_matrix_t M, int rank);
double *fs_dist_y(fs_dist_matrix_t M, int rank);
double *fs_dist_z(fs_dist_matrix_t M, int rank);

/* ---- format construction on the device ------------------------------------------------ */
/* Stable bucketing of host COO entries, the operation behind new_csr / new_bcsr (csr.h:375-422, 30-67: kind 0, key =
 * row), new_cbcsr (cbcsr.h:16-65: kind 1, key = (col / param) * nrow + row) and new_bsbm / new_bsdm (sparse.h:175-213,
 * dsparse.h:132-173: kind 2, key = row / param).  Host arrays in, host arrays out: offsets[nbuckets + 1], and the
 * payload arrays in bucket order with every bucket keeping the input order (rows_out / vals_out may be NULL).  The
 * constructors of include/csr.h, cbcsr.h, sparse.h, dsparse.h call it when fs_device_build_wanted(nnz) says so. */
int fs_bucket_coo(int kind, int param, int nrow, int ncol, int64_t nbuckets, int64_t nnz, const int *rows, const int *cols,
                  const double *vals, int *offsets, int *rows_out, int *cols_out, double *vals_out);
int fs_device_build_wanted(int64_t nnz);

/* ---- side table of layer (1) ---------------------------------------------------------- */
/* forget the device copy made for a host struct (call after mutating its arrays in place) */
void fs_invalidate(const void *host_struct);
/* drop every cached device copy */
void fs_release_all(void);
/* number of device copies currently in the side table.  The table is bounded (FS_DROPIN_MAX_ENTRIES, default 64:
 * the least recently used idle copy goes first) and a copy whose build runs out of HBM is retried after every idle
 * copy has been dropped.  Environment, read once: FS_STRICT_CACHE=1 hashes every host array in full on every call
 * (default: in full up to 8 MB per matrix, 2048 samples per array beyond), FS_DROPIN_CACHE=0 reuses nothing. */
int fs_cache_entries(void);

/* ---- synthetic inputs for bench/tests (counter-based, identical to oracle/fs_synth.c) -- */
/* exactly per_row entries per row, columns uniform on [0,ncol), vals uniform(-1,1) (vals may be NULL) */
int fs_synth_uniform(int nrow, int ncol, int per_row, uint64_t seed, int64_t row_offset,
                     int *row_ptr_dev, int *cols_dev, double *vals_dev, fs_stream_t stream);
/* power-law row lengths (P(len >= L) ~ scale/L, clipped to [1,max_len]) for rows [row_offset, row_offset+nrow) */
int fs_synth_powerlaw_lengths(int nrow, double scale, int max_len, uint64_t seed, int64_t row_offset,
                              int *len_dev, fs_stream_t stream);
/* fill cols/vals for a given row_ptr (uniform columns) */
int fs_synth_fill(int nrow, int ncol, uint64_t seed, int64_t row_offset, const int *row_ptr_dev,
                  int *cols_dev, double *vals_dev, fs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FASTSPARSE_HIP_H */
