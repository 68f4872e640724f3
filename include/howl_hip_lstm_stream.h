/* howl_hip_lstm_stream.h -- streaming seq-lstm / lstm: one kernel launch from N independent PCM chunks to their per-frame class
 * probabilities and the carried recurrent state.
 *
 * Replaces, for the sequential models' inference (howl/model/inference.py:179-211, howl/client/howl_client.py:84-94 and the
 * evaluation loop of the CTC objective), the chain StandardAudioTransform -> ZmuvTransform -> nn.LSTM(40, 128) ->
 * Linear(128, 256) - ReLU - Linear(256, C) -> softmax that howl_logmel_fwd + howl_lstm_fwd + howl_head_fwd + an ATen softmax run
 * as four launches with training-only stores (gates, cell states, hidden sequence) and nine allocations per call.  One workgroup
 * serves four streams and keeps every activation on its compute unit (LDS and registers); nothing couples two streams, so a
 * launch of ceil(N / 4) workgroups serves N independent streams (N = 1 with a carried state: the live client's chunk; N ragged
 * whole clips from a zero state: a dataset pass).
 *
 * Range: M = 40 mel bins, hidden size 128, head 128 -> 256 -> C with 1 <= C <= 64, 400 <= L_max <= 1,638,399 samples (at most
 * 8192 frames), 1 <= N <= 8192, fp32.  Reported by howl_lstm_stream_supported and refused by howl_lstm_stream_chunks; callers
 * keep the launch chain for anything else.
 *
 * Conventions as in howl_hip.h (status codes, howl_last_error, device pointers, caller-owned buffers, one stream).
 */
#ifndef HOWL_HIP_LSTM_STREAM_H
#define HOWL_HIP_LSTM_STREAM_H

#include "howl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOWL_LSTM_STREAM_MAX_STREAMS 8192
#define HOWL_LSTM_STREAM_MAX_CLASSES 64
#define HOWL_LSTM_STREAM_MAX_SAMPLES 1638399 /* 8192 frames: the CTC kernel's longest input */

/* 1 when chunks of up to L_max samples, M mel bins and C classes are inside the kernel's range, else 0. */
int howl_lstm_stream_supported(int L_max, int M, int C);

/* ONE launch of ceil(N / 4) workgroups.  Stream n = pcm[n * ld, n * ld + n_samples[n]) -> log-mel of the WHOLE chunk (standard
 * filterbank `fbp`, howl_fb_from_points / howl_fb_pack; centre framing with reflect padding at the chunk's own two ends, as
 * howl_logmel_fwd on that chunk alone: T_n = 1 + n_samples[n] / 200 frames) -> optional ZMUV (`zmuv_pair` = [mean, std], may be
 * NULL) -> LSTM over frames 0 .. frames[n] - 1 from the state (h[n], c[n]) -> head -> softmax.
 *
 *   n_samples (N) int64 on the device, NULL = L_max for every stream.  Contract: 400 <= n_samples[n] <= L_max; a value outside is
 *             clamped into that range inside the kernel, which therefore reads pcm[n * ld, n * ld + L_max) at most.
 *   frames    (N) int64 on the device, NULL = T_n.  Contract: 1 <= frames[n] <= T_n; a value outside is clamped into that range
 *             inside the kernel (not a launch error: the host never reads the array).
 *   h, c      (N, 128) each, read as the start state and overwritten with the state behind frame frames[n] - 1.  Both NULL: every
 *             stream starts from zeros and the final state is not returned.
 *   last_only 0: probs[n * out_ld + t * C + k] for t < frames[n] are the frame's probabilities and rows frames[n] <= t < T_max
 *             = 1 + L_max / 200 are written as zeros (out_ld >= T_max * C floats per stream);
 *             1: the head runs on the final hidden state only and writes probs[n * out_ld + k] (out_ld >= C).
 *   logits    same layout as probs, the pre-softmax scores; may be NULL.
 * Nothing else of the output buffers is touched.  No prepared state and no workspace: the weights are read in place on every
 * call, so there is nothing that can go stale after load_state_dict.  The weight matrices must be 16-byte aligned. */
int howl_lstm_stream_chunks(const HowlLstmParams* lstm, const HowlHeadParams* head, const float* pcm, long ld, int N, int L_max,
                            const long long* n_samples, const long long* frames, const float* fbp, int M, float log_eps,
                            const float* zmuv_pair, float* h, float* c, int C, int last_only, float* probs, float* logits,
                            long out_ld, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
