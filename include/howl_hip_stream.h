/* howl_hip_stream.h -- streaming res8: one kernel launch from a window's raw PCM to its class probabilities.
 *
 * Replaces, for the live client's window (howl/model/inference.py:247-267, howl/client/howl_client.py:68-94), the chain
 * StandardAudioTransform -> ZmuvTransform -> Res8.forward (eval mode) -> softmax that howl_logmel_fwd + howl_res8_fwd run as about
 * eleven launches.  One workgroup serves one window and keeps every activation on its compute unit (LDS and registers); a launch of
 * N workgroups serves N independent windows (N streams, or N windows of one clip).
 *
 * Range: M = 40 mel bins, windows of 3..83 frames (400 <= L_samples < 16600: up to 1 s), C <= 64 classes, 1 <= N <= 8192.
 * Anything else is reported by howl_res8_stream_supported and refused by the other entry points; callers keep howl_res8_fwd.
 *
 * Conventions as in howl_hip.h (status codes, howl_last_error, device pointers, caller-owned buffers, one stream).
 */
#ifndef HOWL_HIP_STREAM_H
#define HOWL_HIP_STREAM_H

#include "howl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOWL_STREAM_MAX_WINDOWS 8192
#define HOWL_STREAM_MAX_CLASSES 64

/* 1 when windows of L_samples samples, M mel bins and C classes are inside the kernel's range, else 0. */
int howl_res8_stream_supported(int L_samples, int M, int C);

/* Bytes of the prepared state for C classes: the six 3x3 layers' weights as MFMA fragments, conv0's fragments, every BatchNorm's
 * running mean and 1/sqrt(running_var + eps), the output layer. */
size_t howl_res8_stream_state_bytes(int C);

/* One launch: fills `state` from the model's parameters and running buffers.  Run it again whenever one of them changes; the
 * window kernel reads nothing but `state`. */
int howl_res8_stream_prepare(const HowlRes8Params* prm, int C, void* state, size_t state_bytes, hipStream_t stream);

/* ONE launch of N workgroups: window n = pcm[n * ld, n * ld + L_samples) (rows may overlap: ld is the stride between windows) ->
 * log-mel (standard filterbank `fbp`, howl_fb_from_points / howl_fb_pack) -> optional ZMUV (`zmuv_pair` = [mean, std], may be
 * NULL) -> res8 in eval mode -> probs[n, 0:C] = softmax(logits[n, 0:C]).  `logits` may be NULL.  No workspace: the residual map
 * stays in registers, the current map in LDS. */
int howl_res8_stream_windows(const void* state, const float* pcm, long ld, int N, int L_samples, const float* fbp, int M,
                             float log_eps, const float* zmuv_pair, int C, float* probs, float* logits, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
