/* howl_hip_las_stream.h -- streaming las: one kernel launch from a window's raw PCM to its class probabilities.
 *
 * Replaces, for the live client's window (howl/model/inference.py:247-267, howl/client/howl_client.py:68-94), the chain
 * StandardAudioTransform -> deltas -> ZmuvTransform -> LASClassifier.forward (eval mode) -> softmax that howl_logmel_fwd +
 * howl_deltas_fwd + howl_las_fwd run as thirteen launches.  One workgroup serves one window from its first sample to its label;
 * a launch of N workgroups serves N independent windows (N streams, or N windows of one clip).  Nothing is shared between
 * workgroups: window n's bits do not depend on N, on its row index or on its neighbours.
 *
 * The model is the eval-mode model of howl_hip_las.h (BatchNorm from the running statistics, no dropout).  `frames` is the
 * window's compute_lengths: the encoder runs over all T = 1 + L_samples / 200 frames, `frames` only sets the number of recurrence
 * and attention steps, (((frames + 2) / 2) + 2) / 2.
 *
 * Range: M = 40 mel bins, 512 <= L_samples < 16600 (3..83 frames: up to 1 s), 1 <= frames <= T, 1 <= C <= 64 labels,
 * 1 <= N <= 8192.  Anything else is reported by howl_las_stream_supported and refused by the other entry points; callers keep
 * howl_las_fwd.
 *
 * Conventions as in howl_hip.h (status codes, howl_last_error, device pointers, caller-owned buffers, one stream, no
 * synchronisation).  Every refusal happens before the first launch and names the entry point: null pointers, a shape outside the
 * range, a short state, a short workspace (HOWL_E_WORKSPACE).
 */
#ifndef HOWL_HIP_LAS_STREAM_H
#define HOWL_HIP_LAS_STREAM_H

#include "howl_hip_las.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOWL_LAS_STREAM_MAX_WINDOWS 8192

/* 1 when windows of L_samples samples, M mel bins and C labels are inside the kernel's range, else 0. */
int howl_las_stream_supported(int L_samples, int M, int C);

/* Bytes of the prepared state for C labels (0 outside 1..HOWL_LAS_MAX_LABELS): W_ih of both directions and the V / K projections
 * as MFMA B fragments, W_hh in the recurrence's lane order, both BatchNorms folded to scale and shift from the running statistics
 * (eps 1e-5), the conv weights, context_vec and the fc layers. */
size_t howl_las_stream_state_bytes(int C);

/* One launch: fills `state` (16-byte aligned) from the model's parameters and running buffers.  Run it again whenever one of them
 * changes; the window kernel reads the model through `state` alone. */
int howl_las_stream_prepare(const HowlLasParams* prm, const HowlLasBuffers* buffers, int C, void* state, size_t state_bytes,
                            hipStream_t stream);

/* Bytes of `ws` for N windows of L_samples samples (0 outside the range): per window the pooled conv1 map with its zero border and
 * the input projections Gx, each written and read back by the window's own workgroup only. */
size_t howl_las_stream_workspace_bytes(int N, int L_samples);

/* ONE launch of N workgroups: window n = pcm[n * ld, n * ld + L_samples) (rows may overlap: ld is the stride between windows) ->
 * log-mel (standard filterbank `fbp`, howl_fb_from_points / howl_fb_pack), deltas and accelerations -> optional ZMUV (`zmuv_pair` =
 * [mean, std], may be NULL) -> las in eval mode -> probs[n, 0:C] = softmax(logits[n, 0:C]).  `logits` may be NULL.  Nothing
 * outside probs, logits and ws is written. */
int howl_las_stream_windows(const void* state, const float* pcm, long ld, int N, int L_samples, int frames, const float* fbp, int M,
                            float log_eps, const float* zmuv_pair, int C, float* probs, float* logits, void* ws, size_t ws_bytes,
                            hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
