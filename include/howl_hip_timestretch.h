/* howl_hip_timestretch.h -- TimestretchTransform (howl/data/transform/transform.py:146-165) on the device: B independent, ragged
 * clips stretched by a phase vocoder in ONE launch, one 256-thread workgroup per clip.
 *
 * The arithmetic is librosa 0.8's effects.time_stretch(y, rate) (stft with reflect padding, phase_vocoder, istft):
 *   N = 2048, hop 512, periodic Hann w;  yp = reflect_pad(y, 1024);  n_in = 1 + len / 512;  D[:, f] = rfft(yp[512 f ..] w);
 *   step[t] = t * rate in fp64, t < n_out = ceil(n_in / rate);  i = (int)step, a = step - i;
 *   column t = ((1 - a) |D[:, i]| + a |D[:, i + 1]|) exp(j phase[t]),  D[:, f >= n_in] = 0;
 *   exp(j phase[t + 1]) = exp(j phase[t]) u(D[:, i + 1]) conj(u(D[:, i])),  u(z) = z / |z|, u(0) = 1,  exp(j phase[0]) = u(D[:, 0])
 *   (librosa's accumulator phase += phi + wrap(angle(D1) - angle(D0) - phi) with phi[k] = k pi / 2: the same number modulo 2 pi);
 *   out_len = round_half_even(len / rate);  the inverse takes min(n_out, ceil((out_len + 2048) / 512)) columns: irfft(col) w
 *   overlap-added at hop 512, divided by the overlap-added w^2 where that is above FLT_MIN, the first 1024 samples dropped,
 *   cropped or zero padded to out_len.
 * fp32 throughout, except the step index.
 *
 * Conventions as in howl_hip.h (status codes, howl_last_error, device pointers, caller-owned buffers, one stream, no allocation,
 * no synchronisation; every refusal happens before the launch).  No workspace: the state of a clip lives in its workgroup's LDS.
 */
#ifndef HOWL_HIP_TIMESTRETCH_H
#define HOWL_HIP_TIMESTRETCH_H

#include "howl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HOWL_TIMESTRETCH_MAX_CLIPS 8192
#define HOWL_TIMESTRETCH_MIN_SAMPLES 2048     /* a shorter clip is accepted with rate 1.0 only */
#define HOWL_TIMESTRETCH_MAX_SAMPLES 1048576
#define HOWL_TIMESTRETCH_MIN_RATE 0.3
#define HOWL_TIMESTRETCH_MAX_RATE 1.7
/* flag: a clip of rate 1.0 goes through the transform as well (default: it is copied, with its mix) */
#define HOWL_TIMESTRETCH_NO_COPY 1u

/* One clip.  The same 48-byte record is read on the host (to refuse) and on the device (to run). */
typedef struct {
    double rate;         /* exactly 1.0, or in [0.3, 1.7] */
    long long src_row;   /* the clip starts at bank[src_row * bank_ld]: a row of a dense (N, Lmax) bank, or, with bank_ld = 1, an
                            offset into a flat sample buffer -- the two layouts howl_collate_augment_window reads */
    long long dst_off;   /* the stretched clip is out[dst_off .. dst_off + out_len) */
    int len;             /* input samples */
    int out_len;         /* = round_half_even(len / rate): checked */
    int n_out;           /* = ceil((1 + len / 512) / rate), numpy's len(arange(0, n_in, rate)): checked */
    int bg_idx, bg_off;  /* DatasetMixer, applied while reading: y[n] = y[n] (1 - alpha) + bg[bg_idx * bg_ld + bg_off + n] alpha */
    float alpha;         /* 0: no mix for this clip */
} HowlStretchClip;

/* ONE launch of B workgroups.
 *   bank, bank_ld, bank_floats   the clip bank and its size in floats (for the bounds check of every clip)
 *   bg, bg_ld, bg_floats         the background bank of the mix; NULL: every alpha must be 0
 *   clips_host                   HOST, B records: validated here, before the launch
 *   clips_dev                    DEVICE, the same B records: what the kernel reads.  Contract: the bytes of clips_host by the time the
 *                                kernel runs (the caller's copy on `stream`, in front of this call)
 *   out, out_floats              flat destination; clips may not overlap (not checked)
 * Refused: B outside 1 .. 8192, a rate that is neither 1.0 nor in [0.3, 1.7], a rate != 1.0 for a clip under 2048 samples, a clip
 * over HOWL_TIMESTRETCH_MAX_SAMPLES, out_len / n_out that are not the values above, a source, background or destination range
 * outside its buffer. */
int howl_timestretch_clips(const float* bank, long bank_ld, long bank_floats, const float* bg, long bg_ld, long bg_floats,
                           const HowlStretchClip* clips_host, const HowlStretchClip* clips_dev, int B, float* out, long out_floats,
                           unsigned flags, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
