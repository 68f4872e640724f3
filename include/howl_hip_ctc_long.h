/* howl_hip_ctc_long.h -- howl_ctc_loss (howl_hip.h) with the label axis opened: fused log_softmax + CTC loss and its gradient
 * w.r.t. the logits for targets of up to HOWL_CTC_LONG_MAX_LABELS labels.
 *
 * The reference builds its tokenizer with ignore_oov=False, so every word of a transcript is a label, and nn.CTCLoss takes
 * targets of any length (training/run/train.py:250-256,291-296); howl_ctc_loss holds one state of the extended label sequence
 * per lane of a wavefront and stops at 31 labels.  Here a lane holds K consecutive states in registers (K = 2 up to 63 labels,
 * 4 up to 127, 8 up to 255), still one wavefront per utterance; up to 31 labels the call runs howl_ctc_loss's kernel body.
 * Per state and per posterior the arithmetic and its order are howl_ctc_loss's, so an utterance's nll and gradient rows are
 * the same bits whichever of the four bodies runs it: a batch inside howl_ctc_loss's range gives howl_ctc_loss's bits, also
 * when a larger max_target_length is declared.  Everything is fixed-order: repeated calls are bit-identical.
 *
 * Arguments, layouts, the loss (NULL defers the mean) and the per-utterance contract are howl_ctc_loss's, the contract over
 * the whole range: an utterance whose input length is negative, whose target length is negative or above max_target_length,
 * or ANY of whose labels lies outside [0, C) gets nll = +inf and all-zero dlogits rows; only its targets[b][0,
 * max_target_length) are read, and the other utterances' bits are those of the batch with it made valid.
 *
 * An utterance's rows stay in LDS up to howl_ctc_long_window_rows(max_target_length) frames; longer ones are walked in windows
 * of that many frames and, when the gradient is wanted, park their alpha rows in `workspace`:
 * howl_ctc_long_workspace_floats(T, B, max_target_length) floats (0 when T fits one window; workspace may then be NULL).
 *
 * Conventions as in howl_hip.h (status codes, howl_last_error, device pointers, caller-owned buffers, one stream, no
 * synchronisation).  Every refusal happens before the first launch and names this entry point and the limits.
 */
#ifndef HOWL_HIP_CTC_LONG_H
#define HOWL_HIP_CTC_LONG_H

#include "howl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOWL_CTC_LONG_MAX_LABELS 255

/* 1 when 1 <= T <= 8192, 1 <= C <= 64 and 0 <= max_target_length <= 255, else 0. */
int howl_ctc_long_supported(int T, int C, int max_target_length);
/* Frames per LDS window of the kernel body that serves max_target_length: 128 (up to 31 labels), 64 (up to 63), 32 (up to 255);
 * 0 outside the range. */
size_t howl_ctc_long_window_rows(int max_target_length);
/* B * T * 64 * K floats (K = states per lane: 1, 2, 4, 8) when T exceeds the window, else 0. */
size_t howl_ctc_long_workspace_floats(int T, int B, int max_target_length);
int howl_ctc_loss_long(const float* logits, long st_t, long st_b, int T, int B, int C, const long long* targets, long tgt_stride,
                       int max_target_length, const long long* input_lengths, const long long* target_lengths, int blank,
                       float* nll, float* loss, float* dlogits, long dst_t, long dst_b, float* workspace, size_t workspace_floats,
                       hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
