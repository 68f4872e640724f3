// howl_ctc_loss (ctc.hip) for targets beyond 31 labels: include/howl_hip_ctc_long.h.
//
// Still one wavefront per utterance.  Up to 31 labels the launch runs ctc_wave<65>, the body of howl_ctc_loss's kernel (window
// 128, workspace B T 64); beyond, ctc_long_wave<K> (howl_ctc_long.hip.h) with K = 2, 4, 8 states of the extended label sequence
// per lane for up to 63, 127, 255 labels.  The arithmetic per state and per posterior and its order do not depend on the body,
// so a batch inside howl_ctc_loss's range gives howl_ctc_loss's bits whatever max_target_length the caller declares.
// Everything is a fixed-order computation: repeated calls are bit-identical.
#include <math.h>

#include "howl_common.hip.h"
#include "howl_ctc_long.hip.h"
#include "../../include/howl_hip_ctc_long.h"

namespace {

static_assert(CTC_LONG_MAX_L == HOWL_CTC_LONG_MAX_LABELS, "header and kernel disagree");

// up to CTC_MAX_L labels: howl_ctc_loss's kernel body
__global__ __launch_bounds__(64) void ctc_long_k1_kernel(const float* __restrict__ logits, long st_t, long st_b, int T, int B, int C,
                                                         const long long* __restrict__ targets, long tgt_stride, int max_target_length,
                                                         const long long* __restrict__ input_lengths,
                                                         const long long* __restrict__ target_lengths, int blank,
                                                         float* __restrict__ nll_out, float* __restrict__ dlogits, long dst_t,
                                                         long dst_b, int tc, float* __restrict__ alpha_ws) {
    HIP_DYNAMIC_SHARED(float, lds)
    const int b = blockIdx.x;
    ctc_wave<CTC_LONG_CP>(logits + (size_t)b * st_b, st_t, T, B, C, targets + (size_t)b * tgt_stride, (int)input_lengths[b],
                          (int)target_lengths[b], max_target_length, blank, nll_out + b, dlogits ? dlogits + (size_t)b * dst_b : nullptr,
                          dst_t, tc, alpha_ws ? alpha_ws + (size_t)b * T * 64 : nullptr, lds, threadIdx.x);
}

template <int K>
__global__ __launch_bounds__(64) void ctc_long_kernel(const float* __restrict__ logits, long st_t, long st_b, int T, int B, int C,
                                                      const long long* __restrict__ targets, long tgt_stride, int max_target_length,
                                                      const long long* __restrict__ input_lengths,
                                                      const long long* __restrict__ target_lengths, int blank,
                                                      float* __restrict__ nll_out, float* __restrict__ dlogits, long dst_t,
                                                      long dst_b, int tc, float* __restrict__ alpha_ws) {
    HIP_DYNAMIC_SHARED(float, lds)
    const int b = blockIdx.x;
    ctc_long_wave<K>(logits + (size_t)b * st_b, st_t, T, B, C, targets + (size_t)b * tgt_stride, (int)input_lengths[b],
                     (int)target_lengths[b], max_target_length, blank, nll_out + b, dlogits ? dlogits + (size_t)b * dst_b : nullptr,
                     dst_t, tc, alpha_ws ? alpha_ws + (size_t)b * T * 64 * K : nullptr, lds, threadIdx.x);
}

// ctc_mean_kernel's arithmetic (ctc.hip): loss = mean_b nll_b / max(L_b, 1), fixed summation order
__global__ __launch_bounds__(256) void ctc_long_mean_kernel(const float* __restrict__ nll, const long long* __restrict__ target_lengths,
                                                            int B, float* __restrict__ loss) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) {
        const long long L = target_lengths[b];
        acc += (double)(nll[b] / (float)(L > 0 ? L : 1));
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = (float)((((red[0] + red[1]) + red[2]) + red[3]) / (double)B);
}

// states per lane of the body that serves max_target_length (1 = ctc_wave)
int states_per_lane(int max_target_length) {
    return max_target_length <= CTC_MAX_L ? 1 : max_target_length <= CtcLong<2>::MAX_L ? 2 : max_target_length <= CtcLong<4>::MAX_L ? 4 : 8;
}
int window_rows(int k) { return k == 1 ? CTC_CHUNK : k == 2 ? CtcLong<2>::WIN : k == 4 ? CtcLong<4>::WIN : CtcLong<8>::WIN; }

struct CtcLongArgs {
    const float* logits;
    long st_t, st_b;
    int T, B, C;
    const long long* targets;
    long tgt_stride;
    int max_target_length;
    const long long *input_lengths, *target_lengths;
    int blank;
    float *nll, *dlogits;
    long dst_t, dst_b;
    float* ws;
    hipStream_t stream;
};

// false: the runtime refused the LDS (text set, nothing launched, nothing left pending)
template <class Kernel>
bool launch_body(Kernel kernel, size_t lds, size_t* granted, int tc, const CtcLongArgs& a) {
    if (!howl_raise_lds(reinterpret_cast<const void*>(kernel), lds, granted, "howl_ctc_loss_long")) return howl_take_pending_error(), false;
    hipLaunchKernelGGL(kernel, dim3(a.B), dim3(64), lds, a.stream, a.logits, a.st_t, a.st_b, a.T, a.B, a.C, a.targets, a.tgt_stride,
                       a.max_target_length, a.input_lengths, a.target_lengths, a.blank, a.nll, a.dlogits, a.dst_t, a.dst_b, tc, a.ws);
    return true;
}
template <int K>
bool launch_long(int tc, const CtcLongArgs& a) {
    static thread_local size_t granted[16] = {};
    return launch_body(ctc_long_kernel<K>, CtcLong<K>::lds_floats(tc) * sizeof(float), granted, tc, a);
}

}  // namespace

extern "C" {

int howl_ctc_long_supported(int T, int C, int max_target_length) {
    return T >= 1 && T <= CTC_MAX_T && C >= 1 && C <= CTC_MAX_C && max_target_length >= 0 && max_target_length <= CTC_LONG_MAX_L;
}

size_t howl_ctc_long_window_rows(int max_target_length) {
    if (max_target_length < 0 || max_target_length > CTC_LONG_MAX_L) return 0;
    return (size_t)window_rows(states_per_lane(max_target_length));
}

size_t howl_ctc_long_workspace_floats(int T, int B, int max_target_length) {
    if (max_target_length < 0 || max_target_length > CTC_LONG_MAX_L || B <= 0) return 0;
    const int k = states_per_lane(max_target_length);
    return T > window_rows(k) ? (size_t)B * (size_t)T * 64 * (size_t)k : 0;
}

int howl_ctc_loss_long(const float* logits, long st_t, long st_b, int T, int B, int C, const long long* targets, long tgt_stride,
                       int max_target_length, const long long* input_lengths, const long long* target_lengths, int blank,
                       float* nll, float* loss, float* dlogits, long dst_t, long dst_b, float* workspace, size_t workspace_floats,
                       hipStream_t stream) {
    HOWL_REQUIRE(logits && targets && input_lengths && target_lengths && nll, "howl_ctc_loss_long: null pointer");
    HOWL_REQUIRE(B >= 1 && blank >= 0 && blank < C, "howl_ctc_loss_long: bad shape (B=%d, blank=%d, C=%d)", B, blank, C);
    HOWL_REQUIRE(B == 1 || tgt_stride >= max_target_length,
                 "howl_ctc_loss_long: target rows of stride %ld overlap (max_target_length %d)", tgt_stride, max_target_length);
    HOWL_REQUIRE(howl_ctc_long_supported(T, C, max_target_length),
                 "howl_ctc_loss_long: T=%d C=%d target length %d outside the kernel's range (T <= %d, C <= %d, targets <= %d)", T,
                 C, max_target_length, CTC_MAX_T, CTC_MAX_C, CTC_LONG_MAX_L);
    const int k = states_per_lane(max_target_length), win = window_rows(k);
    const size_t need = howl_ctc_long_workspace_floats(T, B, max_target_length);
    const bool spills = dlogits != nullptr && T > win;     // the loss alone keeps nothing of the alpha rows
    HOWL_REQUIRE(!spills || (workspace && workspace_floats >= need),
                 "howl_ctc_loss_long: T=%d > %d frames with a gradient and targets <= %d labels needs a workspace of "
                 "howl_ctc_long_workspace_floats(T, B, max_target_length) = %zu floats (got %zu)", T, win, max_target_length, need,
                 workspace ? workspace_floats : (size_t)0);
    const int tc = T < win ? T : win;
    const CtcLongArgs a{logits, st_t, st_b, T, B, C, targets, tgt_stride, max_target_length, input_lengths, target_lengths, blank,
                        nll, dlogits, dst_t, dst_b, spills ? workspace : (float*)nullptr, stream};
    bool ok;
    if (k == 1) {
        static thread_local size_t granted[16] = {};
        ok = launch_body(ctc_long_k1_kernel, ((size_t)4 * tc * CTC_LONG_CP + 64) * sizeof(float), granted, tc, a);
    } else {
        ok = k == 2 ? launch_long<2>(tc, a) : k == 4 ? launch_long<4>(tc, a) : launch_long<8>(tc, a);
    }
    if (!ok) return HOWL_E_LAUNCH;
    if (loss != nullptr)     // NULL: the caller takes the batch mean elsewhere (howl_head_bwd's HowlCtcMean: one launch fewer)
        hipLaunchKernelGGL(ctc_long_mean_kernel, dim3(1), dim3(256), 0, stream, (const float*)nll, target_lengths, B, loss);
    HOWL_CHECK_LAUNCH("howl_ctc_loss_long");
    return HOWL_OK;
}

}  // extern "C"
