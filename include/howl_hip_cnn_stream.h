/* howl_hip_cnn_stream.h -- streaming small-cnn and seq-cnn: one kernel launch from raw PCM to class probabilities.
 *
 * Replaces the chain StandardAudioTransform -> ZmuvTransform -> SmallCnn / SequentialCnn.forward (eval mode) -> softmax that
 * howl_logmel_fwd + howl_cnn_fwd run as eight launches and torch finishes with a ninth:
 *   small-cnn: the live client's window (howl/model/inference.py:247-267).  One workgroup serves one window from its first sample
 *              to its label; a launch of N workgroups serves N independent windows (N streams, or N windows of one clip).
 *   seq-cnn:   InferenceEngine.infer's chunk and a dataset pass of the CTC objective (inference.py:179-211).  One workgroup serves
 *              one (clip, tile of HOWL_CNN_STREAM_TILE_ROWS output rows) pair and computes everything the tile needs itself, the
 *              halo included (8 R + 25 frames for R rows); a launch serves N ragged clips.
 * Nothing is shared between workgroups: the bits of a window or of a clip do not depend on N, on its row index, on its neighbours,
 * on L_max or on ld.
 *
 * The model is the eval-mode model of howl_hip_cnn.h (BatchNorm from the running statistics, no dropout).  There is no prepared
 * state: the kernel reads HowlCnnParams and the running statistics of HowlCnnBuffers in place, as howl_cnn_fwd does, so nothing can
 * go stale (bn1_batches / bn2_batches are not read and may be NULL).
 *
 * Range: M = 40 mel bins, 1 <= C <= 64 labels, 1 <= N <= 8192, fp32.  T = 1 + L_samples / 200 frames:
 *   HOWL_CNN_SMALL: 26 <= T <= 41, i.e. 5000 <= L_samples <= 8199 (the client's 500 ms window is 8000 samples, 41 frames);
 *   HOWL_CNN_SEQ:   5 <= T <= 8192, i.e. 800 <= L_samples <= 1638399; a clip has r = howl_cnn_stream_rows output rows,
 *                   r rows exactly for 1600 r - 800 <= L_samples <= 1600 r + 799.
 * Anything else is reported by howl_cnn_stream_supported and refused by the two launches; callers keep howl_cnn_fwd.
 *
 * Conventions as in howl_hip.h (status codes, howl_last_error, device pointers, caller-owned buffers, one stream, no
 * synchronisation).  Every refusal happens before the first launch and names the entry point: null pointers, the other kind's
 * launch, a shape outside the range, out_ld below what the launch writes, a short workspace (HOWL_E_WORKSPACE).
 */
#ifndef HOWL_HIP_CNN_STREAM_H
#define HOWL_HIP_CNN_STREAM_H

#include "howl_hip_cnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOWL_CNN_STREAM_MAX_WINDOWS 8192
/* output rows one workgroup of the seq-cnn kernel produces */
#define HOWL_CNN_STREAM_TILE_ROWS 8

/* 1 when rows of L_samples samples, M mel bins and C labels are inside the range of `kind`'s launch, else 0. */
int howl_cnn_stream_supported(int kind, int L_samples, int M, int C);

/* Bytes of `ws` for N rows of up to L_max samples (0 outside the range, else a positive multiple of 16).  The kernel keeps
 * everything in LDS: the answer inside the range is 16. */
size_t howl_cnn_stream_workspace_bytes(int kind, int N, int L_max);

/* Output rows of an L_samples-sample clip: howl_cnn_out_rows(kind, 1 + L_samples / 200); 0 outside the range. */
size_t howl_cnn_stream_rows(int kind, int L_samples);

/* small-cnn.  ONE launch of N workgroups: window n = pcm[n * ld, n * ld + L_samples) (rows may overlap: ld is the stride between
 * windows) -> log-mel (standard filterbank `fbp`, howl_fb_from_points / howl_fb_pack) -> optional ZMUV (`zmuv_pair` = [mean, std],
 * may be NULL) -> small-cnn in eval mode -> probs[n, 0:C] = softmax(logits[n, 0:C]).  `logits` may be NULL.  Nothing outside probs,
 * logits and ws is written. */
int howl_cnn_stream_windows(const HowlCnnParams* prm, const HowlCnnBuffers* buffers, const float* pcm, long ld, int N, int L_samples,
                            const float* fbp, int M, float log_eps, const float* zmuv_pair, int C, float* probs, float* logits,
                            void* ws, size_t ws_bytes, hipStream_t stream);

/* seq-cnn.  ONE launch: clip n = pcm[n * ld, n * ld + n_samples[n]) -> log-mel -> optional ZMUV -> seq-cnn in eval mode ->
 * probs[n * out_ld + r * C + k] = softmax over k of the logits of output row r, for r < howl_cnn_stream_rows(n_samples[n]); the rows
 * from there up to howl_cnn_stream_rows(L_max) are written as zeros.  `n_samples`: int64 on the device, NULL = L_max for every
 * clip; a value outside [800, L_max] is clamped inside the kernel.  out_ld >= howl_cnn_stream_rows(L_max) * C.  `logits` has the
 * layout of `probs` and may be NULL.  Nothing outside probs, logits and ws is written. */
int howl_cnn_stream_clips(const HowlCnnParams* prm, const HowlCnnBuffers* buffers, const float* pcm, long ld, int N, int L_max,
                          const long long* n_samples, const float* fbp, int M, float log_eps, const float* zmuv_pair, int C,
                          float* probs, float* logits, long out_ld, void* ws, size_t ws_bytes, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
