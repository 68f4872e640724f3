// The tests' door to the dense kernels of howl_gemm.hip.h: include/howl_hip_dense.h.
//
// Nothing here computes: every entry point checks its arguments, clears the header's choice log, calls the header's host helper
// with the caller's arguments and leaves the log for howl_dense_choices.  The one kernel of this file is the 512-thread wrapper
// that runs wgrad_w8_body per block (in the product that body rides in the LSTM's backward recurrence launch).  This translation
// unit compiles its own copy of the header: same source and flags as the models', not the same code object.
#include "howl_common.hip.h"
#include "howl_gemm.hip.h"
#include "../../include/howl_hip_dense.h"

namespace {

static_assert(HOWL_DENSE_LIN == BIG, "header and kernels disagree");
static_assert(HOWL_DENSE_MAX_CHOICES == DENSE_LOG_MAX, "header and kernels disagree");
static_assert(HOWL_DENSE_MAX_SLAB_JOBS == MAX_SLAB_JOBS && HOWL_DENSE_MAX_WGRAD_JOBS == MAX_WGRAD_JOBS, "header and kernels disagree");
static_assert(sizeof(HowlDenseChoice) == sizeof(DenseChoice), "header and kernels disagree");
static_assert(HOWL_DENSE_GEMM == DC_GEMM && HOWL_DENSE_GEMM_VEC == DC_GEMM_VEC && HOWL_DENSE_ROWGEMM == DC_ROWGEMM &&
                  HOWL_DENSE_THIN_WGRAD == DC_THIN_WGRAD && HOWL_DENSE_WGRAD_BIG == DC_WGRAD_BIG && HOWL_DENSE_WGRAD_JOB == DC_WGRAD_JOB &&
                  HOWL_DENSE_WGRAD_MULTI == DC_WGRAD_MULTI && HOWL_DENSE_WGRAD_W8 == DC_WGRAD_W8 && HOWL_DENSE_SUM_SLABS == DC_SUM_SLABS &&
                  HOWL_DENSE_SUM_SLABS_MULTI == DC_SUM_SLABS_MULTI && HOWL_DENSE_COLSUM == DC_COLSUM && HOWL_DENSE_RELU_BWD == DC_RELU_BWD,
              "header and kernels disagree");

RowMap rm_of(const HowlDenseRowMap& r) { return RowMap{r.inner, r.s_outer, r.s_inner}; }
bool rm_ok(const HowlDenseRowMap& r) { return r.inner >= 1; }

// one block of a collected 128 x 128 job per 512-thread workgroup
__global__ __launch_bounds__(512) void dense_w8_kernel(WgradJob jb) {
    __shared__ __attribute__((aligned(16))) float As[2][WG_K * WG_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[2][WG_K * WG_LDA];
    wgrad_w8_body(jb, (int)blockIdx.x, As, Bs);
}

// What wgrad_gemm / wgrad_dual_gemm will do with a job: the number of slabs (0: a dual job that does not fit) and whether the
// 128-row kernel takes it.  The tests allocate exactly splits * n floats between guards, so a disagreement with the helpers shows.
struct WgradPlan {
    int splits;
    bool big;
};
WgradPlan wgrad_plan(const HowlDenseWgrad& j) {
    auto map4 = [](const HowlDenseRowMap& r) { return (r.s_outer & 3) == 0 && (r.s_inner & 3) == 0; };
    auto al16 = [](const float* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool big_rows = j.n_out >= 128 && j.rows >= wgrad_big_min_rows() && (j.n_out & 3) == 0 && map4(j.dm) && map4(j.im) && al16(j.dout) &&
                          al16(j.in) && j.max_splits >= 16;
    auto big_splits = [&](int tiles) {
        int sp = std::max(1, howl_num_cus() / tiles);
        sp = std::min(sp, j.max_splits);
        int kps = ((j.rows + sp - 1) / sp + WG_K - 1) / WG_K * WG_K;
        kps = std::max(kps, 4 * WG_K);
        return (j.rows + kps - 1) / kps;
    };
    if (j.in2 != nullptr) {
        const bool fits = big_rows && j.k_in == 128 && j.k2 >= 4 && j.k2 <= 64 && (j.k2 & 3) == 0 && map4(j.im2) && al16(j.in2) &&
                          getenv("HOWL_WGRAD_NO_DUAL") == nullptr;
        return WgradPlan{fits ? big_splits((j.n_out + WG_M - 1) / WG_M) : 0, fits};
    }
    int splits = j.rows / j.rows_per_split;
    splits = splits < 1 ? 1 : (splits > j.max_splits ? j.max_splits : splits);
    if (j.n_out <= 8 && ((j.n_out & 3) != 0 || (j.k_in & 3) != 0)) {
        const int rpc = (j.rows + splits - 1) / splits;
        return WgradPlan{(j.rows + rpc - 1) / rpc, false};
    }
    if (big_rows && (j.k_in & 3) == 0 && j.k_in >= 16) {
        const int tn = j.k_in > 64 ? 128 : 64;
        return WgradPlan{big_splits(((j.n_out + WG_M - 1) / WG_M) * ((j.k_in + tn - 1) / tn)), true};
    }
    const int kps = ((j.rows + splits - 1) / splits + GK - 1) / GK * GK;
    return WgradPlan{(j.rows + kps - 1) / kps, false};
}

// nullptr: fine; otherwise the reason
const char* wgrad_bad(const HowlDenseWgrad& j) {
    if (!(j.dout && j.in && j.scratch && j.dw)) return "null pointer";
    if (!(j.n_out >= 1 && j.k_in >= 1 && j.rows >= 1 && j.max_splits >= 1 && j.rows_per_split >= 1)) return "bad shape";
    if (!(rm_ok(j.dm) && rm_ok(j.im))) return "row map with inner < 1";
    if (j.in2 != nullptr) {
        if (!(j.scratch2 && j.dw2)) return "null pointer";
        if (!rm_ok(j.im2)) return "row map with inner < 1";
    }
    return nullptr;
}

// every launching entry point starts a new record
void choices_reset() { dense_log.n = 0; }

}  // namespace

extern "C" {

size_t howl_dense_choices(HowlDenseChoice* out, size_t max) {
    const size_t n = (size_t)dense_log.n;
    for (size_t i = 0; out != nullptr && i < n && i < max; ++i) {
        const DenseChoice& e = dense_log.e[i];
        out[i] = HowlDenseChoice{e.family, e.t0, e.t1, e.t2, e.t3, e.gx, e.gy, e.gz, e.kps};
    }
    return n;
}

size_t howl_dense_num_cus(void) { return (size_t)howl_num_cus(); }

size_t howl_dense_gemm_splits(int K, int splits) {
    if (K < 1 || splits < 1) return 0;
    const int kps = ((K + splits - 1) / splits + GK - 1) / GK * GK;
    return (size_t)((K + kps - 1) / kps);
}

size_t howl_dense_gemm_c_floats(const HowlDenseGemm* g) {
    if (g == nullptr || g->M < 1 || g->N < 1 || g->c_ms < 0 || g->c_split_stride < 0) return 0;
    const size_t z = howl_dense_gemm_splits(g->K, g->splits);
    return z == 0 ? 0 : (z - 1) * (size_t)g->c_split_stride + (size_t)(g->M - 1) * (size_t)g->c_ms + (size_t)g->N;
}

int howl_dense_gemm(const HowlDenseGemm* g, int* splits_out, int* thin_done, hipStream_t stream) {
    HOWL_REQUIRE(g != nullptr && g->a && g->b && g->c, "howl_dense_gemm: null pointer");
    HOWL_REQUIRE(g->M >= 1 && g->N >= 1 && g->K >= 1 && g->splits >= 1, "howl_dense_gemm: bad shape (M=%d, N=%d, K=%d, splits=%d)", g->M,
                 g->N, g->K, g->splits);
    HOWL_REQUIRE(rm_ok(g->am) && rm_ok(g->ak) && rm_ok(g->bk), "howl_dense_gemm: row map with inner < 1");
    HOWL_REQUIRE(g->c_ms >= g->N, "howl_dense_gemm: rows of c overlap (c_ms=%ld < N=%d)", g->c_ms, g->N);
    const size_t z = howl_dense_gemm_splits(g->K, g->splits);
    HOWL_REQUIRE(z == 1 || g->c_split_stride >= (long)(g->M - 1) * g->c_ms + g->N, "howl_dense_gemm: slabs of c overlap (c_split_stride=%ld)",
                 g->c_split_stride);
    const size_t need = howl_dense_gemm_c_floats(g);
    HOWL_REQUIRE(g->c_floats >= need, "howl_dense_gemm: c needs howl_dense_gemm_c_floats = %zu floats (got %zu)", need, g->c_floats);
    HOWL_REQUIRE(g->thin_out >= 0 && g->thin_out <= 8, "howl_dense_gemm: thin_out=%d outside 0..8", g->thin_out);
    HOWL_REQUIRE(g->thin_out == 0 || (g->w2 && g->b2 && g->y2), "howl_dense_gemm: null pointer (second layer)");
    choices_reset();
    const RowGemmThin thin{g->w2, g->b2, g->y2};
    bool done = false;
    const int zz = gemm(stream, g->a_major_k != 0, g->a, rm_of(g->am), g->a_ks, rm_of(g->ak), g->b, rm_of(g->bk), g->b_ns, g->M, g->N, g->K,
                        g->splits, g->bias, g->relu, g->c, g->c_ms, g->c_split_stride, g->thin_out > 0 ? &thin : nullptr, g->thin_out, &done);
    if (splits_out != nullptr) *splits_out = zz;
    if (thin_done != nullptr) *thin_done = done ? 1 : 0;
    HOWL_CHECK_LAUNCH("howl_dense_gemm");
    return HOWL_OK;
}

size_t howl_dense_wgrad_splits(const HowlDenseWgrad* j) {
    if (j == nullptr || wgrad_bad(*j) != nullptr) return 0;
    return (size_t)wgrad_plan(*j).splits;
}
size_t howl_dense_wgrad_scratch_floats(const HowlDenseWgrad* j) { return howl_dense_wgrad_splits(j) * (size_t)j->n_out * (size_t)j->k_in; }
size_t howl_dense_wgrad_scratch2_floats(const HowlDenseWgrad* j) {
    return j != nullptr && j->in2 != nullptr ? howl_dense_wgrad_splits(j) * (size_t)j->n_out * (size_t)j->k2 : 0;
}

int howl_dense_wgrad(int form, int njobs, const HowlDenseWgrad* jobs, hipStream_t stream) {
    HOWL_REQUIRE(form >= 0 && form <= 2, "howl_dense_wgrad: form=%d outside 0..2", form);
    HOWL_REQUIRE(jobs != nullptr && njobs >= 1 && njobs <= 8, "howl_dense_wgrad: njobs=%d outside 1..8", njobs);
    for (int q = 0; q < njobs; ++q) {
        const HowlDenseWgrad& j = jobs[q];
        const char* bad = wgrad_bad(j);
        HOWL_REQUIRE(bad == nullptr, "howl_dense_wgrad: job %d: %s", q, bad);
        HOWL_REQUIRE(j.in2 == nullptr || form == 2, "howl_dense_wgrad: job %d: the dual job needs form 2 (collected)", q);
        const WgradPlan p = wgrad_plan(j);
        HOWL_REQUIRE(p.splits >= 1,
                     "howl_dense_wgrad: job %d: the dual job does not fit (n_out=%d k_in=%d k2=%d rows=%d max_splits=%d: needs n_out >= 128, "
                     "k_in = 128, k2 in 4..64, multiples of 4, 16-byte aligned operands, max_splits >= 16, rows >= the 128-row threshold)",
                     q, j.n_out, j.k_in, j.k2, j.rows, j.max_splits);
        const size_t need = (size_t)p.splits * j.n_out * j.k_in;
        HOWL_REQUIRE(j.scratch_floats >= need, "howl_dense_wgrad: job %d: scratch needs howl_dense_wgrad_scratch_floats = %zu floats (got %zu)", q,
                     need, j.scratch_floats);
        const size_t need2 = j.in2 != nullptr ? (size_t)p.splits * j.n_out * j.k2 : 0;
        HOWL_REQUIRE(j.in2 == nullptr || j.scratch2_floats >= need2,
                     "howl_dense_wgrad: job %d: scratch2 needs howl_dense_wgrad_scratch2_floats = %zu floats (got %zu)", q, need2, j.scratch2_floats);
    }
    if (form == 2) {      // a dual job is refused once the collector is full: count the jobs in front of it that the 128-row kernel takes
        int collected = 0;
        for (int q = 0; q < njobs; ++q) {
            const bool big = wgrad_plan(jobs[q]).big;
            HOWL_REQUIRE(jobs[q].in2 == nullptr || collected < MAX_WGRAD_JOBS, "howl_dense_wgrad: job %d: the dual job behind %d collected jobs", q,
                         collected);
            if (big && collected < MAX_WGRAD_JOBS) ++collected;
        }
    }
    choices_reset();
    SlabSums sums;
    WgradJobs collected;
    for (int q = 0; q < njobs; ++q) {
        const HowlDenseWgrad& j = jobs[q];
        if (j.in2 != nullptr) {
            const bool ok = wgrad_dual_gemm(j.dout, rm_of(j.dm), j.n_out, j.in, rm_of(j.im), j.in2, rm_of(j.im2), j.k2, j.rows, j.scratch, j.dw,
                                            j.scratch2, j.dw2, j.max_splits, &sums, &collected);
            if (!ok) {      // (the plan said it fits)
                howl_set_error("howl_dense_wgrad: job %d: wgrad_dual_gemm refused a job the plan accepted", q);
                return HOWL_E_ARG;
            }
            continue;
        }
        wgrad_gemm(stream, j.dout, rm_of(j.dm), j.n_out, j.in, rm_of(j.im), j.k_in, j.rows, j.scratch, j.dw, j.max_splits, j.rows_per_split,
                   form >= 1 ? &sums : nullptr, form == 2 ? &collected : nullptr);
    }
    if (form == 2) wgrad_jobs_flush(stream, collected);
    if (form >= 1 && !sums.flush(stream)) return HOWL_E_ARG;
    HOWL_CHECK_LAUNCH("howl_dense_wgrad");
    return HOWL_OK;
}

int howl_dense_wgrad_slabs(const HowlDenseWgrad* jp, int eight_waves, int* splits_out, hipStream_t stream) {
    HOWL_REQUIRE(jp != nullptr, "howl_dense_wgrad_slabs: null pointer");
    const HowlDenseWgrad& j = *jp;
    const char* bad = wgrad_bad(j);
    HOWL_REQUIRE(bad == nullptr, "howl_dense_wgrad_slabs: %s", bad);
    HOWL_REQUIRE(j.in2 == nullptr, "howl_dense_wgrad_slabs: a single job only");
    const WgradPlan p = wgrad_plan(j);
    HOWL_REQUIRE(p.big && j.k_in > 64,
                 "howl_dense_wgrad_slabs: not a 128-column job of the 128-row kernel (n_out=%d k_in=%d rows=%d max_splits=%d: needs n_out >= 128, "
                 "k_in > 64, multiples of 4, 16-byte aligned operands, max_splits >= 16, rows >= the 128-row threshold)",
                 j.n_out, j.k_in, j.rows, j.max_splits);
    const size_t need = (size_t)p.splits * j.n_out * j.k_in;
    HOWL_REQUIRE(j.scratch_floats >= need, "howl_dense_wgrad_slabs: scratch needs howl_dense_wgrad_scratch_floats = %zu floats (got %zu)", need,
                 j.scratch_floats);
    choices_reset();
    SlabSums sums;      // the fold is queued and dropped: slabs only
    WgradJobs collected;
    wgrad_gemm(stream, j.dout, rm_of(j.dm), j.n_out, j.in, rm_of(j.im), j.k_in, j.rows, j.scratch, j.dw, j.max_splits, j.rows_per_split, &sums,
               &collected);
    if (collected.count != 1 || collected.j[0].tn != 128) {
        howl_set_error("howl_dense_wgrad_slabs: wgrad_gemm did not collect the job the plan accepted");
        return HOWL_E_ARG;
    }
    const WgradJob& jb = collected.j[0];
    if (splits_out != nullptr) *splits_out = jb.gz;
    if (eight_waves) {
        dense_note(DC_WGRAD_W8, 128, 0, 0, 0, dim3(wgrad_job_blocks(jb)), jb.kps);
        hipLaunchKernelGGL(dense_w8_kernel, dim3(wgrad_job_blocks(jb)), dim3(512), 0, stream, jb);
    } else {
        dense_note(DC_WGRAD_BIG, 128, 0, 0, 0, dim3(jb.gx, jb.gy, jb.gz), jb.kps);
        hipLaunchKernelGGL((wgrad_big_kernel<128, false>), dim3(jb.gx, jb.gy, jb.gz), dim3(WG_THREADS), 0, stream, jb.dout, jb.dm, jb.in, jb.im,
                           jb.M, jb.N, jb.K, jb.kps, jb.part);
    }
    HOWL_CHECK_LAUNCH("howl_dense_wgrad_slabs");
    return HOWL_OK;
}

size_t howl_dense_colsum_chunks(int rows, int max_chunks, int rows_per_chunk) {
    if (rows < 1 || max_chunks < 1 || rows_per_chunk < 1) return 0;
    int chunks = rows / rows_per_chunk;
    chunks = chunks < 1 ? 1 : (chunks > max_chunks ? max_chunks : chunks);
    return (size_t)chunks;
}

int howl_dense_colsum(const float* x, const HowlDenseRowMap* rm, int rows, int n, float* scratch, size_t scratch_floats, float* out0,
                      float* out1, int max_chunks, int rows_per_chunk, int deferred, hipStream_t stream) {
    HOWL_REQUIRE(x && rm && scratch && out0, "howl_dense_colsum: null pointer");
    HOWL_REQUIRE(rows >= 1 && n >= 1 && max_chunks >= 1 && rows_per_chunk >= 1 && rm_ok(*rm),
                 "howl_dense_colsum: bad shape (rows=%d, n=%d, max_chunks=%d, rows_per_chunk=%d, inner=%d)", rows, n, max_chunks, rows_per_chunk,
                 rm->inner);
    const size_t need = howl_dense_colsum_chunks(rows, max_chunks, rows_per_chunk) * (size_t)n;
    HOWL_REQUIRE(scratch_floats >= need, "howl_dense_colsum: scratch needs howl_dense_colsum_chunks * n = %zu floats (got %zu)", need,
                 scratch_floats);
    choices_reset();
    SlabSums sums;
    colsum(stream, x, rm_of(*rm), rows, n, scratch, out0, out1, max_chunks, rows_per_chunk, deferred ? &sums : nullptr);
    if (deferred && !sums.flush(stream)) return HOWL_E_ARG;
    HOWL_CHECK_LAUNCH("howl_dense_colsum");
    return HOWL_OK;
}

int howl_dense_slab_sums(int njobs, const HowlDenseSlabJob* jobs, const HowlAdamW* adamw, const HowlCtcMean* mean, hipStream_t stream) {
    HOWL_REQUIRE(njobs >= 0 && (njobs == 0 || jobs != nullptr), "howl_dense_slab_sums: null pointer");
    HOWL_REQUIRE(njobs > 0 || mean != nullptr, "howl_dense_slab_sums: nothing to do");
    for (int q = 0; q < njobs; ++q) {
        const HowlDenseSlabJob& j = jobs[q];
        HOWL_REQUIRE(j.part && j.out, "howl_dense_slab_sums: job %d: null pointer", q);
        HOWL_REQUIRE(j.nparts >= 1 && j.n >= 1 && j.stride >= j.n, "howl_dense_slab_sums: job %d: bad shape (nparts=%d, n=%ld, stride=%ld)", q,
                     j.nparts, j.n, j.stride);
        if (adamw != nullptr)
            for (const float* o : {(const float*)j.out, (const float*)j.out2})
                HOWL_REQUIRE(o == nullptr || (o >= adamw->g && o + j.n <= adamw->g + adamw->n),
                             "howl_dense_slab_sums: job %d: an output outside the optimiser's gradient buffer", q);
    }
    HOWL_REQUIRE(adamw == nullptr || (adamw->p && adamw->g && adamw->m && adamw->v && adamw->step >= 1),
                 "howl_dense_slab_sums: null pointer or step < 1 (adamw)");
    HOWL_REQUIRE(mean == nullptr || (mean->nll && mean->target_lengths && mean->loss && mean->B >= 1),
                 "howl_dense_slab_sums: null pointer or B < 1 (mean)");
    choices_reset();
    SlabSums sums;
    for (int q = 0; q < njobs; ++q) sums.add_strided(jobs[q].part, jobs[q].nparts, jobs[q].stride, jobs[q].n, jobs[q].out, jobs[q].out2);
    if (mean != nullptr) sums.mean = SlabMean{mean->nll, mean->target_lengths, mean->B, mean->loss};
    SlabAdamW opt{nullptr, nullptr, nullptr, nullptr, HowlAdamWCoef{}, 0};
    if (adamw != nullptr)
        opt = SlabAdamW{adamw->p, adamw->g, adamw->m, adamw->v,
                        howl_adamw_coef(adamw->lr, adamw->beta1, adamw->beta2, adamw->eps, adamw->weight_decay, adamw->step, adamw->grad_scale), 1};
    if (!sums.flush(stream, adamw != nullptr ? &opt : nullptr)) return HOWL_E_ARG;      // overflow: the collector's message, nothing launched
    HOWL_CHECK_LAUNCH("howl_dense_slab_sums");
    return HOWL_OK;
}

int howl_dense_sum_slabs(const float* part, int nparts, long n, float* out, hipStream_t stream) {
    HOWL_REQUIRE(part && out, "howl_dense_sum_slabs: null pointer");
    HOWL_REQUIRE(nparts >= 1 && n >= 1, "howl_dense_sum_slabs: bad shape (nparts=%d, n=%ld)", nparts, n);
    choices_reset();
    dense_note(DC_SUM_SLABS, 0, 0, 0, 0, dim3((unsigned)((n + 63) / 64)), nparts);
    hipLaunchKernelGGL(sum_slabs_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, stream, part, nparts, n, out);
    HOWL_CHECK_LAUNCH("howl_dense_sum_slabs");
    return HOWL_OK;
}

int howl_dense_relu_bwd(const float* dy, const float* y, long n, float* dz, hipStream_t stream) {
    HOWL_REQUIRE(dy && y && dz, "howl_dense_relu_bwd: null pointer");
    HOWL_REQUIRE(n >= 1, "howl_dense_relu_bwd: bad shape (n=%ld)", n);
    choices_reset();
    const unsigned blocks = (unsigned)std::min<long>(1024, (n + 255) / 256);      // (the head launches 1024 blocks: a grid-stride loop)
    dense_note(DC_RELU_BWD, 0, 0, 0, 0, dim3(blocks), 0);
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(blocks), dim3(256), 0, stream, dy, y, n, dz);
    HOWL_CHECK_LAUNCH("howl_dense_relu_bwd");
    return HOWL_OK;
}

}  // extern "C"
