/* howl_hip_gru_stream.h -- streaming gru: one kernel launch from a window's raw PCM to its class probabilities.
 *
 * Replaces, for the live client's window (howl/model/inference.py:247-267, howl/client/howl_client.py:68-94), the chain
 * StandardAudioTransform -> ZmuvTransform -> SimpleGru.forward (eval mode) -> softmax that howl_logmel_fwd + howl_gru_fwd run as
 * four launches and torch finishes with a fifth.  One workgroup serves one window from its first sample to its label; a launch of
 * N workgroups serves N independent windows (N streams, or N windows of one clip).  Nothing is shared between workgroups: window
 * n's bits do not depend on N, on its row index or on its neighbours.
 *
 * The model is the eval-mode model of howl_hip_gru.h (BatchNorm from the running statistics, no dropout).  There is no prepared
 * state: the kernel reads HowlGruParams and the running statistics of HowlGruBuffers in place, as howl_gru_fwd does, so nothing can
 * go stale (bn1_batches / bn2_batches are not read and may be NULL).  `frames` is the window's compute_lengths: the encoder runs
 * over all T = 1 + L_samples / 200 frames, `frames` only sets the number of recurrence steps, min((frames + 4) / 2, (T + 4) / 2).
 *
 * Range: M = 40 mel bins, 512 <= L_samples < 16600 (3..83 frames: up to 1 s), 1 <= frames <= T, 1 <= C <= 64 labels,
 * 1 <= N <= 8192.  Anything else is reported by howl_gru_stream_supported and refused by howl_gru_stream_windows; callers keep
 * howl_gru_fwd.
 *
 * Conventions as in howl_hip.h (status codes, howl_last_error, device pointers, caller-owned buffers, one stream, no
 * synchronisation).  Every refusal happens before the first launch and names the entry point: null pointers, a shape outside the
 * range, a short workspace (HOWL_E_WORKSPACE).
 */
#ifndef HOWL_HIP_GRU_STREAM_H
#define HOWL_HIP_GRU_STREAM_H

#include "howl_hip_gru.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOWL_GRU_STREAM_MAX_WINDOWS 8192

/* 1 when windows of L_samples samples, M mel bins and C labels are inside the kernel's range, else 0. */
int howl_gru_stream_supported(int L_samples, int M, int C);

/* Bytes of `ws` for N windows of L_samples samples (0 outside the range, else a positive multiple of 16): per window the pooled
 * conv1 map with its zero border, written and read back by the window's own workgroup only. */
size_t howl_gru_stream_workspace_bytes(int N, int L_samples);

/* ONE launch of N workgroups: window n = pcm[n * ld, n * ld + L_samples) (rows may overlap: ld is the stride between windows) ->
 * log-mel (standard filterbank `fbp`, howl_fb_from_points / howl_fb_pack) -> optional ZMUV (`zmuv_pair` = [mean, std], may be
 * NULL) -> gru in eval mode -> probs[n, 0:C] = softmax(logits[n, 0:C]).  `logits` may be NULL.  Nothing outside probs, logits and
 * ws is written. */
int howl_gru_stream_windows(const HowlGruParams* prm, const HowlGruBuffers* buffers, const float* pcm, long ld, int N, int L_samples,
                            int frames, const float* fbp, int M, float log_eps, const float* zmuv_pair, int C, float* probs,
                            float* logits, void* ws, size_t ws_bytes, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
