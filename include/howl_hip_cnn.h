/* howl_hip_cnn.h -- the "small-cnn" and "seq-cnn" models (howl/model/cnn.py:32-104, SmallCnn / SequentialCnn) as one call per
 * direction.  Both share one encoder on the (time, frequency) view of the 40 log-Mel bins:
 *   conv0 (1 -> 48; HOWL_CNN_SMALL: kernel (8 t, 16 f), pad (4, 0), stride (2, 2); HOWL_CNN_SEQ: kernel (20, 16), pad (10, 0),
 *   stride (1, 2)) - ReLU - MaxPool 2x2 (floor) - BatchNorm2d(48)
 *   - Conv2d(48, 64, 5x5, pad 2, stride (2, 1)) - ReLU - MaxPool 2x2 - BatchNorm2d(64)            -> (64, H, 3)
 * and differ in the head's rows:
 *   HOWL_CNN_SMALL: H == 2 (26 <= T <= 41); flatten (c, h, w) - Linear(384,128) - ReLU - Dropout - Linear(128, L) -> (B, L)
 *   HOWL_CNN_SEQ:   per output row t: flatten (c, w) - Linear(192,128) - ReLU - Dropout - Linear(128, L)         -> (B, H, L)
 * with H = howl_cnn_out_rows(kind, T).
 *
 * x: element (b, mel, t) at x[b*sb + mel*sm + t*st], the log-Mel channel of the (B, C, 40, T) features.  The whole buffer goes
 * through the encoder, padded frames included (they count in the BatchNorm statistics, as in the reference).
 *
 * training != 0: batch statistics (biased variance to normalise; the running buffers are updated with momentum 0.1 and the
 * unbiased variance, num_batches_tracked += 1) and, when drop_mask (0/1; HOWL_CNN_SMALL: (B, 128), HOWL_CNN_SEQ: (H, B, 128)) is
 * given, y1 * mask * keep_scale between the head's ReLU and its second layer; everything howl_cnn_bwd needs stays in `ws`, which
 * must reach that call untouched.  training == 0: running statistics; drop_mask must be NULL.
 *
 * logits: (B, L) or (B, H, L).  howl_cnn_bwd: dlogits of the same shape -> every entry of `grads` written (no input gradient).
 * Fixed-order sums everywhere: repeated calls are bit-identical, and an utterance's eval-mode logits do not depend on its batch
 * neighbours.  The max-pool passes its gradient to the first maximum in scan order.
 *
 * Conventions as in howl_hip.h (status codes, howl_last_error, device pointers, caller-owned buffers, one stream, no
 * synchronisation).  Every refusal happens before the first launch and names the entry point: null pointers, an unknown kind,
 * M != 40, T outside the kind's range (small: 26..41, seq: 5..HOWL_CNN_MAX_FRAMES), B < 1, B * H beyond 2^20 head rows,
 * num_labels outside 1..HOWL_CNN_MAX_LABELS, a short workspace (HOWL_E_WORKSPACE).
 */
#ifndef HOWL_HIP_CNN_H
#define HOWL_HIP_CNN_H

#include "howl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOWL_CNN_SMALL 0
#define HOWL_CNN_SEQ 1
#define HOWL_CNN_MAX_FRAMES 8192
#define HOWL_CNN_MAX_LABELS 64

typedef struct {
    const float* conv0_w; /* encoder1.0.weight (48,1,KT,16), KT = 8 (small) or 20 (seq) */
    const float* conv0_b; /* encoder1.0.bias (48) */
    const float* bn1_w;   /* encoder1.3.weight (48) */
    const float* bn1_b;   /* encoder1.3.bias (48) */
    const float* conv1_w; /* encoder2.0.weight (64,48,5,5) */
    const float* conv1_b; /* encoder2.0.bias (64) */
    const float* bn2_w;   /* encoder2.3.weight (64) */
    const float* bn2_b;   /* encoder2.3.bias (64) */
    const float* w1;      /* output.0.weight (128, 384 or 192) */
    const float* b1;      /* output.0.bias (128) */
    const float* w2;      /* output.3.weight (num_labels,128) */
    const float* b2;      /* output.3.bias (num_labels) */
} HowlCnnParams;

/* the same twelve tensors, in the same order */
typedef struct {
    float *conv0_w, *conv0_b, *bn1_w, *bn1_b, *conv1_w, *conv1_b, *bn2_w, *bn2_b, *w1, *b1, *w2, *b2;
} HowlCnnGrads;

/* BatchNorm buffers, updated in place when training */
typedef struct {
    float* bn1_mean;        /* encoder1.3.running_mean (48) */
    float* bn1_var;         /* encoder1.3.running_var (48) */
    long long* bn1_batches; /* encoder1.3.num_batches_tracked (1) */
    float* bn2_mean;        /* encoder2.3.running_mean (64) */
    float* bn2_var;         /* encoder2.3.running_var (64) */
    long long* bn2_batches; /* encoder2.3.num_batches_tracked (1) */
} HowlCnnBuffers;

/* 1 when the problem is inside the limits above, else 0. */
int howl_cnn_supported(int kind, int B, int M, int T, int num_labels);
/* Bytes of `ws` for the problem: saved activations, gradients in flight and partial sums (0 outside the range). */
size_t howl_cnn_workspace_bytes(int kind, int B, int T, int num_labels);
/* Rows H of the encoder's output for T frames (0 when T is outside the kind's range); SequentialCnn.compute_length(T). */
size_t howl_cnn_out_rows(int kind, int T);
int howl_cnn_fwd(int kind, const HowlCnnParams* p, const HowlCnnBuffers* buffers, const float* x, long sb, long sm, long st, int B,
                 int M, int T, int num_labels, int training, const float* drop_mask, float keep_scale, float* logits, void* ws,
                 size_t ws_bytes, hipStream_t stream);
int howl_cnn_bwd(int kind, const HowlCnnParams* p, const float* x, long sb, long sm, long st, int B, int M, int T, int num_labels,
                 float keep_scale, const float* dlogits, const HowlCnnGrads* grads, void* ws, size_t ws_bytes, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
