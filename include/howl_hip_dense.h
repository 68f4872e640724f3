/* howl_hip_dense.h -- a door to the dense kernels of howl_amd/csrc/howl_gemm.hip.h for the tests.
 *
 * The generic fp32 MFMA GEMM (64 x 64 tiles, scalar and 16-byte loads), the weights-stationary GEMM for tall row sets with its
 * thin second layer, the thin and the 128-row weight-gradient kernels (one launch, several collected jobs in one launch, the dual
 * job, the eight-wave body), the deterministic slab folds with their AdamW and CTC-mean riders, the column sums and the ReLU
 * backward all sit in an anonymous namespace behind the models.  These entry points call the header's HOST HELPERS (gemm,
 * wgrad_gemm, wgrad_dual_gemm, wgrad_jobs_flush, colsum, SlabSums) with every argument they take, so a test can run each kernel
 * instance at edge shapes on operands it placed itself, and read back which instance the dispatcher chose.
 *
 * Limitation: every translation unit that includes howl_gemm.hip.h compiles its own copy.  What runs here is dense.hip's copy:
 * the same source and the same compiler flags as lstm.hip's, gru.hip's, las.hip's, cnn.hip's and mobilenet.hip's, not the same
 * code object.
 *
 * Row maps: row x of an operand starts at element (x / inner) * s_outer + (x % inner) * s_inner; inner = HOWL_DENSE_LIN makes it
 * the plain stride x * s_inner.  Dispatch thresholds are read from the environment on every call (HOWL_ROWGEMM_MIN_ROWS,
 * HOWL_WGRAD_BIG_MIN_ROWS; default 2048 rows).
 *
 * Conventions as in howl_hip.h (status codes, howl_last_error, device pointers, caller-owned buffers, one stream, no
 * synchronisation).  Every refusal happens before the first launch and names the entry point and the reason: null pointers, bad
 * shapes, an output or scratch region smaller than the matching size query says.  The entry points trust strides and row maps:
 * the caller answers for the operands covering what the maps address.
 */
#ifndef HOWL_HIP_DENSE_H
#define HOWL_HIP_DENSE_H

#include "howl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOWL_DENSE_LIN (1 << 30)
#define HOWL_DENSE_MAX_CHOICES 16
#define HOWL_DENSE_MAX_SLAB_JOBS 8
#define HOWL_DENSE_MAX_WGRAD_JOBS 4

typedef struct {
    int inner;
    long s_outer, s_inner;
} HowlDenseRowMap;

/* kernel families of a choice record */
#define HOWL_DENSE_GEMM 1             /* gemm_kernel<t0 = A_MAJOR_IS_K> */
#define HOWL_DENSE_GEMM_VEC 2         /* gemm_vec_kernel<t0 = A_UNIT_K, t1 = B_UNIT_K, t2 = KMAP_LIN> */
#define HOWL_DENSE_ROWGEMM 3          /* rowgemm_kernel<t0 = KG, t1 = NT, t2 = W_UNIT_K, t3 = NO2> */
#define HOWL_DENSE_THIN_WGRAD 4       /* thin_wgrad_kernel<t0 = NO>; kps = rows per chunk */
#define HOWL_DENSE_WGRAD_BIG 5        /* wgrad_big_kernel<t0 = TN, t1 = KMAP_LIN> */
#define HOWL_DENSE_WGRAD_JOB 6        /* a job collected for wgrad_big_multi_kernel: t0 = 64, 128, 192 (dual), t1 = KMAP_LIN */
#define HOWL_DENSE_WGRAD_MULTI 7      /* wgrad_big_multi_kernel's launch: t0 = jobs, gx = blocks */
#define HOWL_DENSE_WGRAD_W8 8         /* wgrad_w8_body, one block of the job per 512-thread workgroup */
#define HOWL_DENSE_SUM_SLABS 9        /* sum_slabs_kernel; kps = slabs */
#define HOWL_DENSE_SUM_SLABS_MULTI 10 /* sum_slabs_multi_kernel: t0 = jobs, t1 = AdamW rider, t2 = mean rider */
#define HOWL_DENSE_COLSUM 11          /* colsum_kernel; kps = rows per chunk */
#define HOWL_DENSE_RELU_BWD 12        /* relu_bwd_kernel */

/* One launch (or one collected job): the kernel family, its template arguments, the grid, and k (rows) per split where the
 * family splits its reduction. */
typedef struct {
    int family, t0, t1, t2, t3, gx, gy, gz, kps;
} HowlDenseChoice;
/* The records of this thread's last howl_dense_* launching call, in launch order: writes min(count, max) of them, returns count. */
size_t howl_dense_choices(HowlDenseChoice* out, size_t max);
/* Workgroups the persistent kernels spread over (the device's compute units). */
size_t howl_dense_num_cus(void);

/* C[m][n] = sum_k A(m,k) B(k,n) (+ bias[n]) (ReLU), split z of the reduction to c + z * c_split_stride.
 *   a_major_k: A(m,k) = a[am(m) + k * a_ks], else a[am(m) + ak(k)];  B(k,n) = b[bk(k) + n * b_ns].
 * thin_out 1..8 offers a second layer y2 (M, thin_out) = C w2^T + b2 (w2 (thin_out, N) packed); *thin_done tells whether it
 * rode along. */
typedef struct {
    int a_major_k;
    const float* a;
    HowlDenseRowMap am;
    long a_ks;
    HowlDenseRowMap ak;
    const float* b;
    HowlDenseRowMap bk;
    long b_ns;
    int M, N, K, splits;
    const float* bias; /* NULL: none */
    int relu;
    float* c;
    long c_ms, c_split_stride;
    size_t c_floats; /* floats behind c */
    const float* w2;
    const float* b2;
    float* y2;
    int thin_out; /* 0: no second layer */
} HowlDenseGemm;
/* Slabs the 64 x 64 kernels write for (K, splits); 1 whenever the weights-stationary kernel runs (it takes splits = 1 only). */
size_t howl_dense_gemm_splits(int K, int splits);
/* (slabs - 1) * c_split_stride + (M - 1) * c_ms + N */
size_t howl_dense_gemm_c_floats(const HowlDenseGemm* g);
int howl_dense_gemm(const HowlDenseGemm* g, int* splits_out, int* thin_done, hipStream_t stream);

/* dw (n_out, k_in) = dOut^T In over `rows` mapped rows: split slabs in scratch, then a deterministic fold.
 * in2 != NULL: the dual job, dw2 (n_out, k2) = dOut^T In2 as well, k_in = 128 (form 2 only). */
typedef struct {
    const float* dout;
    HowlDenseRowMap dm;
    int n_out;
    const float* in;
    HowlDenseRowMap im;
    int k_in, rows;
    float* scratch;
    size_t scratch_floats;
    float* dw;
    int max_splits, rows_per_split;
    const float* in2; /* NULL: a single job */
    HowlDenseRowMap im2;
    int k2;
    float* scratch2;
    size_t scratch2_floats;
    float* dw2;
} HowlDenseWgrad;
/* Slabs the job writes (depends on the pointers' alignment, the maps and the environment, like the dispatch itself); 0 when the
 * dual job does not fit. */
size_t howl_dense_wgrad_splits(const HowlDenseWgrad* j);
/* splits * n_out * k_in, and splits * n_out * k2 for the second product of a dual job */
size_t howl_dense_wgrad_scratch_floats(const HowlDenseWgrad* j);
size_t howl_dense_wgrad_scratch2_floats(const HowlDenseWgrad* j);
/* form 0: every job launches and folds at once (sum_slabs_kernel).  form 1: the folds are deferred into one SlabSums and flushed
 * once.  form 2: as 1, and jobs that the 128-row kernel takes are collected (up to HOWL_DENSE_MAX_WGRAD_JOBS; a further one
 * launches on its own) and launched together by wgrad_jobs_flush.  1 <= njobs <= 8; more than HOWL_DENSE_MAX_SLAB_JOBS folds
 * fail with the collector's overflow message after the products have run. */
int howl_dense_wgrad(int form, int njobs, const HowlDenseWgrad* jobs, hipStream_t stream);
/* One job that the 128-row kernel takes with 128-column tiles (k_in > 64), slabs only (no fold): eight_waves = 1 runs
 * wgrad_w8_body per block of a 512-thread kernel, 0 runs wgrad_big_kernel<128, false> on the same grid and split. */
int howl_dense_wgrad_slabs(const HowlDenseWgrad* j, int eight_waves, int* splits_out, hipStream_t stream);

/* out0 (and out1, may be NULL) = column sums of x (rows mapped by rm, n columns); scratch: chunks * n floats. */
size_t howl_dense_colsum_chunks(int rows, int max_chunks, int rows_per_chunk);
int howl_dense_colsum(const float* x, const HowlDenseRowMap* rm, int rows, int n, float* scratch, size_t scratch_floats, float* out0,
                      float* out1, int max_chunks, int rows_per_chunk, int deferred, hipStream_t stream);

/* SlabSums::add_strided per job, then flush: out[i] (and out2[i]) = sum over g < nparts of part[g * stride + i], i < n.
 * adamw != NULL: the step rides in the fold (every out / out2 must lie in [adamw->g, adamw->g + adamw->n)); mean != NULL: the CTC
 * batch mean rides as one more block row. */
typedef struct {
    const float* part;
    int nparts;
    long stride, n;
    float* out;
    float* out2; /* NULL: none */
} HowlDenseSlabJob;
int howl_dense_slab_sums(int njobs, const HowlDenseSlabJob* jobs, const HowlAdamW* adamw, const HowlCtcMean* mean, hipStream_t stream);
/* sum_slabs_kernel alone: out[i] = sum over g < nparts of part[g * n + i] */
int howl_dense_sum_slabs(const float* part, int nparts, long n, float* out, hipStream_t stream);

/* dz[i] = y[i] > 0 ? dy[i] : 0; dz may be dy */
int howl_dense_relu_bwd(const float* dy, const float* y, long n, float* dz, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
