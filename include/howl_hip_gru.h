/* howl_hip_gru.h -- the "gru" classifier (howl/model/rnn.py:94-130, SimpleGru) as one call per direction:
 *   Conv2d(1,8,3,padding=(1,3)) - BatchNorm2d(8) - ReLU - MaxPool(1,2) - Conv2d(8,1,3,padding=1) - ReLU - BatchNorm2d(1)
 *   - GRU(40 -> 96), packed, final hidden state - Linear(96,192) - ReLU - Dropout - Linear(192, num_labels).
 *
 * x: element (b, mel, t) at x[b*sb + mel*sm + t*st], the log-Mel channel of the (B, C, 40, T) features.  The whole buffer goes
 * through the encoder, padded frames included (they count in the BatchNorm statistics, as in the reference); `lengths` (B,
 * int64, NULL = T for all) only decides where each recurrence stops: utterance b runs min((lengths[b] + 4) / 2, (T + 4) / 2)
 * steps.  Nothing is written to `lengths`.
 *
 * training != 0: batch statistics (biased variance to normalise; the running buffers are updated with momentum 0.1 and the
 * unbiased variance, num_batches_tracked += 1) and, when drop_mask (B, 192 of 0/1) is given, y1 * mask * keep_scale between
 * the head's ReLU and its second layer; everything howl_gru_bwd needs stays in `ws`, which must reach that call untouched.
 * training == 0: running statistics, nothing saved; drop_mask must be NULL.
 *
 * howl_gru_bwd: dlogits (B, num_labels) -> every entry of `grads` written (no input gradient).  Fixed-order sums everywhere:
 * repeated calls are bit-identical, and an utterance's eval-mode logits do not depend on its batch neighbours.
 *
 * Conventions as in howl_hip.h (status codes, howl_last_error, device pointers, caller-owned buffers, one stream, no
 * synchronisation).  Every refusal happens before the first launch and names the entry point: null pointers, M != 40,
 * T outside 1..HOWL_GRU_MAX_FRAMES, B < 1, num_labels outside 1..HOWL_GRU_MAX_LABELS, a short workspace (HOWL_E_WORKSPACE).
 */
#ifndef HOWL_HIP_GRU_H
#define HOWL_HIP_GRU_H

#include "howl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOWL_GRU_MAX_FRAMES 8192
#define HOWL_GRU_MAX_LABELS 64

typedef struct {
    const float* conv1_w; /* conv_encoder.0.weight (8,1,3,3) */
    const float* conv1_b; /* conv_encoder.0.bias (8) */
    const float* bn1_w;   /* conv_encoder.1.weight (8) */
    const float* bn1_b;   /* conv_encoder.1.bias (8) */
    const float* conv2_w; /* conv_encoder.4.weight (1,8,3,3) */
    const float* conv2_b; /* conv_encoder.4.bias (1) */
    const float* bn2_w;   /* conv_encoder.6.weight (1) */
    const float* bn2_b;   /* conv_encoder.6.bias (1) */
    const float* w_ih;    /* lstm_encoder.weight_ih_l0 (288,40), rows r | z | n */
    const float* w_hh;    /* lstm_encoder.weight_hh_l0 (288,96) */
    const float* b_ih;    /* lstm_encoder.bias_ih_l0 (288) */
    const float* b_hh;    /* lstm_encoder.bias_hh_l0 (288) */
    const float* w1;      /* dnn.0.weight (192,96) */
    const float* b1;      /* dnn.0.bias (192) */
    const float* w2;      /* dnn.3.weight (num_labels,192) */
    const float* b2;      /* dnn.3.bias (num_labels) */
} HowlGruParams;

/* the same sixteen tensors, in the same order */
typedef struct {
    float *conv1_w, *conv1_b, *bn1_w, *bn1_b, *conv2_w, *conv2_b, *bn2_w, *bn2_b, *w_ih, *w_hh, *b_ih, *b_hh, *w1, *b1, *w2, *b2;
} HowlGruGrads;

/* BatchNorm buffers, updated in place when training */
typedef struct {
    float* bn1_mean;        /* conv_encoder.1.running_mean (8) */
    float* bn1_var;         /* conv_encoder.1.running_var (8) */
    long long* bn1_batches; /* conv_encoder.1.num_batches_tracked (1) */
    float* bn2_mean;        /* conv_encoder.6.running_mean (1) */
    float* bn2_var;         /* conv_encoder.6.running_var (1) */
    long long* bn2_batches; /* conv_encoder.6.num_batches_tracked (1) */
} HowlGruBuffers;

/* 1 when B >= 1, M == 40, 1 <= T <= 8192 and 1 <= num_labels <= 64, else 0. */
int howl_gru_supported(int B, int M, int T, int num_labels);
/* Bytes of `ws` for problem (B, T): saved activations, gradients in flight and partial sums (0 outside the range). */
size_t howl_gru_workspace_bytes(int B, int T);
int howl_gru_fwd(const HowlGruParams* p, const HowlGruBuffers* buffers, const float* x, long sb, long sm, long st, int B, int M,
                 int T, int num_labels, const long long* lengths, int training, const float* drop_mask, float keep_scale,
                 float* logits, void* ws, size_t ws_bytes, hipStream_t stream);
int howl_gru_bwd(const HowlGruParams* p, const float* x, long sb, long sm, long st, int B, int M, int T, int num_labels,
                 const long long* lengths, float keep_scale, const float* dlogits, const HowlGruGrads* grads, void* ws,
                 size_t ws_bytes, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
