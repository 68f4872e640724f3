// TimestretchTransform on the device (include/howl_hip_timestretch.h): a phase vocoder over B ragged clips in ONE launch, one
// 256-thread workgroup per clip, which walks the clip's output frames in order.  Nothing is shared between clips.
//
// Per output frame t (step = t * rate in fp64, i = (int)step, a = step - i):
//   1. the spectra D[:, i] and D[:, i + 1] live in two LDS slots (frame f in slot f & 1) and are recomputed only when i advances:
//      window the reflect-padded (and mixed) samples, pack them as 1024 complex points, FFT, split step -> 1025 bins;
//   2. every lane carries the unit phasor of its bins k = lane + 256 j in registers (bin 1024 is lane 0's fifth): the output column
//      is mag * p, then p <- normalise(p u(D1) conj(u(D0))) -- no atan2, no sincos, and |p| stays 1;
//   3. inverse split step, inverse FFT, window, overlap-add into a ring of 2048 samples; the 512 samples no later frame touches are
//      divided by the w^2 envelope (up to four table terms, from the frame index) and stored.
// The 1024-point FFT is five radix-4 decimation-in-time stages in place (input in base-4 digit-reversed order, one butterfly per
// lane and stage, a barrier between stages); twiddles, split-step factors and the Hann window all come from one table of
// W_2048^k (howl_timestretch_tables.h), whose first 1536 entries are copied into LDS when the workgroup starts.
//
// The FORWARD transform carries every value as an unevaluated sum of two floats (hi, lo; error-free TwoSum / fma products, about
// 2^-44 relative), the table's rounding residues included, and rounds once when it stores a spectrum.  Plain fp32 butterflies are
// not enough there: the phase of a bin is D / |D|, and every rounding of a butterfly that still holds the clip's strong partials
// lands, at eps x THEIR magnitude, in bins that are a thousand times weaker -- measured on the test clips (0.25 sine + 0.05 noise)
// 3e-6 per bin against 6e-8 for a transform that rounds once, which at rate 0.3 is 15 .. 20 x the gap between the float32 and
// float64 statements of the algorithm in the output.  A weak bin's phase error does not average out: u(D[:, f]) enters the phasor
// k1 times as a factor and k2 times as a conjugate factor, and k1 != k2 whenever the rate is not 1.  The inverse transform has no
// such amplification (its error is eps x the output's own magnitude) and stays plain fp32.
//
// LDS (static): table 12,288; two spectra 16,400; column 8,200; FFT buffer 16,384 (two-float forward; its first half is the inverse's
// buffer); overlap-add ring 8,192: 61,464 bytes.
#include <float.h>

#include "howl_common.hip.h"
#include "howl_timestretch_tables.h"
#include "../../include/howl_hip_timestretch.h"

namespace {

constexpr int TS_N = 2048;            // samples per frame
constexpr int TS_HOP = 512;
constexpr int TS_C = TS_N / 2;        // complex points of the packed transform
constexpr int TS_BINS = TS_C + 1;
constexpr int TS_THREADS = 256;
constexpr int TS_TAB = 3 * TS_N / 4;  // table entries in LDS: twiddle indices stay below 3 * 512, the window folds at 1024
static_assert(TS_C == 4 * TS_THREADS && TS_C == 1 << 10, "one radix-4 butterfly per lane and stage, five stages");

struct TsArgs {
    const float* bank;
    long bank_ld;
    const float* bg;
    long bg_ld;
    const HowlStretchClip* clips;
    float* out;
    unsigned flags;
};

// base-4 digit reversal of a 10-bit index
__device__ __forceinline__ int ts_rev4(int k) {
    return ((k & 3) << 8) | (((k >> 2) & 3) << 6) | (((k >> 4) & 3) << 4) | (((k >> 6) & 3) << 2) | ((k >> 8) & 3);
}
__device__ __forceinline__ float2 ts_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 ts_cmul_conj(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }   // a conj(b)
__device__ __forceinline__ float ts_abs(float2 z) { return sqrtf(z.x * z.x + z.y * z.y); }
// u(z) = z / |z|, u(0) = 1 (correctly rounded divisions: the build has no fast-math flag)
__device__ __forceinline__ float2 ts_unit(float2 z, float m) { return m > 0.0f ? make_float2(z.x / m, z.y / m) : make_float2(1.0f, 0.0f); }

// sample m of the clip, with DatasetMixer's mix -- collate_augment_kernel's expression, without contraction, so that a mixed
// read and a read of a bank mixed beforehand give the same bits
__device__ __forceinline__ float ts_sample(const float* __restrict__ src, const float* __restrict__ bsrc, float al, int m) {
#pragma clang fp contract(off)
    float v = src[m];
    if (bsrc != nullptr) v = v * (1.0f - al) + bsrc[m] * al;
    return v;
}

// cos(2 pi n / 2048) is even about n = 1024: the periodic Hann window 0.5 - 0.5 cos from the first 1025 table entries
__device__ __forceinline__ int ts_fold(int n) { return n <= TS_C ? n : TS_N - n; }
__device__ __forceinline__ float ts_hann(const float2* tab, int n) { return 0.5f - 0.5f * tab[ts_fold(n)].x; }

// ---- two-float arithmetic of the forward transform (no contraction may touch the error terms) ----
struct TsDf {
    float hi, lo;
};
struct TsDc {
    TsDf re, im;
};
__device__ __forceinline__ TsDf ts_df_add(TsDf a, TsDf b) {
#pragma clang fp contract(off)
    const float s = a.hi + b.hi, bb = s - a.hi;
    float e = (a.hi - (s - bb)) + (b.hi - bb);       // TwoSum: s + e == a.hi + b.hi exactly
    e += a.lo + b.lo;
    const float hi = s + e;
    return TsDf{hi, e - (hi - s)};
}
__device__ __forceinline__ TsDf ts_df_neg(TsDf a) { return TsDf{-a.hi, -a.lo}; }
__device__ __forceinline__ TsDf ts_df_sub(TsDf a, TsDf b) { return ts_df_add(a, ts_df_neg(b)); }
__device__ __forceinline__ TsDf ts_df_half(TsDf a) { return TsDf{0.5f * a.hi, 0.5f * a.lo}; }
__device__ __forceinline__ TsDf ts_df_mul(TsDf a, TsDf b) {
#pragma clang fp contract(off)
    const float p = a.hi * b.hi;
    float e = fmaf(a.hi, b.hi, -p);                  // p + e == a.hi * b.hi exactly
    e = fmaf(a.hi, b.lo, e);
    e = fmaf(a.lo, b.hi, e);
    const float hi = p + e;
    return TsDf{hi, e - (hi - p)};
}
__device__ __forceinline__ TsDc ts_dc_mul(TsDc a, TsDc w) {
    return TsDc{ts_df_sub(ts_df_mul(a.re, w.re), ts_df_mul(a.im, w.im)), ts_df_add(ts_df_mul(a.re, w.im), ts_df_mul(a.im, w.re))};
}
__device__ __forceinline__ TsDc ts_dc_add(TsDc a, TsDc b) { return TsDc{ts_df_add(a.re, b.re), ts_df_add(a.im, b.im)}; }
__device__ __forceinline__ TsDc ts_dc_sub(TsDc a, TsDc b) { return TsDc{ts_df_sub(a.re, b.re), ts_df_sub(a.im, b.im)}; }
__device__ __forceinline__ TsDc ts_dc_load(const float4* buf, int i) {
    const float4 v = buf[i];
    return TsDc{TsDf{v.x, v.y}, TsDf{v.z, v.w}};
}
__device__ __forceinline__ void ts_dc_store(float4* buf, int i, TsDc z) { buf[i] = make_float4(z.re.hi, z.re.lo, z.im.hi, z.im.lo); }
// W_2048^k as a two-float pair: the rounded value from LDS, its residue from the constant table
__device__ __forceinline__ TsDc ts_dc_twiddle(const float2* tab, int k) {
    const float2 w = tab[k];
    return TsDc{TsDf{w.x, HOWL_TS_W2048_LO[2 * k]}, TsDf{w.y, HOWL_TS_W2048_LO[2 * k + 1]}};
}

// The forward 1024-point FFT in two-float arithmetic: buf holds (re.hi, re.lo, im.hi, im.lo), base-4 digit-reversed input,
// natural output.  Starts and ends with a workgroup barrier.
__device__ __forceinline__ void ts_fft1024_forward(float4* buf, const float2* tab) {
    const int j = threadIdx.x;
    for (int s = 0; s < 5; ++s) {
        const int q = 1 << (2 * s);
        const int pos = j & (q - 1);
        const int i0 = ((j >> (2 * s)) << (2 * s + 2)) + pos;
        __syncthreads();
        TsDc a0 = ts_dc_load(buf, i0), a1 = ts_dc_load(buf, i0 + q), a2 = ts_dc_load(buf, i0 + 2 * q), a3 = ts_dc_load(buf, i0 + 3 * q);
        if (s > 0) {
            const int ts = pos * (TS_N / (4 * q));
            a1 = ts_dc_mul(a1, ts_dc_twiddle(tab, ts)), a2 = ts_dc_mul(a2, ts_dc_twiddle(tab, 2 * ts)), a3 = ts_dc_mul(a3, ts_dc_twiddle(tab, 3 * ts));
        }
        const TsDc t0 = ts_dc_add(a0, a2), t1 = ts_dc_sub(a0, a2), t2 = ts_dc_add(a1, a3), t3 = ts_dc_sub(a1, a3);
        const TsDc it3 = TsDc{t3.im, ts_df_neg(t3.re)};            // -i t3
        ts_dc_store(buf, i0, ts_dc_add(t0, t2));
        ts_dc_store(buf, i0 + q, ts_dc_add(t1, it3));
        ts_dc_store(buf, i0 + 2 * q, ts_dc_sub(t0, t2));
        ts_dc_store(buf, i0 + 3 * q, ts_dc_sub(t1, it3));
    }
    __syncthreads();
}

// In-place 1024-point FFT of buf (base-4 digit-reversed input, natural output).  INV: conjugate twiddles, unnormalised.  Starts
// and ends with a workgroup barrier.
template <bool INV>
__device__ __forceinline__ void ts_fft1024(float2* buf, const float2* tab) {
    const int j = threadIdx.x;
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int q = 1 << (2 * s);                  // a quarter of this stage's span L = 4 q
        const int pos = j & (q - 1);
        const int i0 = ((j >> (2 * s)) << (2 * s + 2)) + pos;
        __syncthreads();
        float2 a0 = buf[i0], a1 = buf[i0 + q], a2 = buf[i0 + 2 * q], a3 = buf[i0 + 3 * q];
        if (s > 0) {
            const int ts = pos * (TS_N / (4 * q));   // W_L^pos = W_2048^(pos 2048 / L); 3 ts < 1536
            float2 w1 = tab[ts], w2 = tab[2 * ts], w3 = tab[3 * ts];
            if (INV) w1.y = -w1.y, w2.y = -w2.y, w3.y = -w3.y;
            a1 = ts_cmul(a1, w1), a2 = ts_cmul(a2, w2), a3 = ts_cmul(a3, w3);
        }
        const float2 t0 = make_float2(a0.x + a2.x, a0.y + a2.y), t1 = make_float2(a0.x - a2.x, a0.y - a2.y);
        const float2 t2 = make_float2(a1.x + a3.x, a1.y + a3.y), t3 = make_float2(a1.x - a3.x, a1.y - a3.y);
        // forward: y1 = t1 - i t3, y3 = t1 + i t3; inverse: the other way round
        const float2 it3 = INV ? make_float2(-t3.y, t3.x) : make_float2(t3.y, -t3.x);
        buf[i0] = make_float2(t0.x + t2.x, t0.y + t2.y);
        buf[i0 + q] = make_float2(t1.x + it3.x, t1.y + it3.y);
        buf[i0 + 2 * q] = make_float2(t0.x - t2.x, t0.y - t2.y);
        buf[i0 + 3 * q] = make_float2(t1.x - it3.x, t1.y - it3.y);
    }
    __syncthreads();
}

__global__ __launch_bounds__(TS_THREADS) void timestretch_kernel(TsArgs a) {
    __shared__ float2 tab[TS_TAB];
    __shared__ float2 spec[2][TS_BINS];
    __shared__ float2 col[TS_BINS];
    __shared__ float4 workd[TS_C];                                    // the forward transform's two-float points
    __shared__ float ring[TS_N];
    float2* const work = reinterpret_cast<float2*>(workd);            // the inverse transform's points

    const int tid = threadIdx.x;
    const HowlStretchClip c = a.clips[blockIdx.x];
    const int len = c.len, out_len = c.out_len;
    const float* __restrict__ src = a.bank + c.src_row * a.bank_ld;
    const float al = a.bg != nullptr ? c.alpha : 0.0f;
    const float* __restrict__ bsrc = al != 0.0f ? a.bg + (long)c.bg_idx * a.bg_ld + c.bg_off : nullptr;
    float* __restrict__ dst = a.out + c.dst_off;

    if (c.rate == 1.0 && !(a.flags & HOWL_TIMESTRETCH_NO_COPY)) {      // TimestretchTransform at rate 1: the clip (mixed) as it is
        for (int n = tid; n < out_len; n += TS_THREADS) dst[n] = n < len ? ts_sample(src, bsrc, al, n) : 0.0f;
        return;
    }

    for (int k = tid; k < TS_TAB; k += TS_THREADS) tab[k] = make_float2(HOWL_TS_W2048[2 * k], HOWL_TS_W2048[2 * k + 1]);
    __syncthreads();

    const int n_in = 1 + len / TS_HOP;
    const int by_len = (out_len + TS_N + TS_HOP - 1) / TS_HOP;
    const int n_used = c.n_out < by_len ? c.n_out : by_len;           // columns the inverse transform takes
    int cached0 = -1, cached1 = -1;                                   // the frame each spectrum slot holds
    float2 p[5];                                                      // unit phasors of bins tid + 256 j
#pragma unroll
    for (int j = 0; j < 5; ++j) p[j] = make_float2(1.0f, 0.0f);

    // the 512 t .. 512 t + count samples of the padded output are final: envelope, crop, store
    auto retire = [&](int s0, int count) {
        for (int r = tid; r < count; r += TS_THREADS) {
            const int s = s0 + r, o = s - TS_C;
            if (o < 0 || o >= out_len) continue;
            const int fs = s / TS_HOP;
            const int f_lo = fs - 3 > 0 ? fs - 3 : 0, f_hi = fs < n_used - 1 ? fs : n_used - 1;
            float wss = 0.0f;
            for (int f = f_lo; f <= f_hi; ++f) {
                const float w = ts_hann(tab, s - TS_HOP * f);
                wss += w * w;
            }
            const float v = ring[s & (TS_N - 1)];
            dst[o] = wss > FLT_MIN ? v / wss : v;
        }
    };

    for (int t = 0; t < n_used; ++t) {
        const double step = (double)t * c.rate;                        // np.arange(0, n_in, rate)[t], in fp64
        const int i = (int)step;
        const float af = (float)(step - (double)i);

        // ---- 1. D[:, i] and D[:, i + 1] ----
        for (int e = 0; e < 2; ++e) {
            const int f = i + e, slot = f & 1;
            if ((slot ? cached1 : cached0) == f) continue;
            if (slot) cached1 = f; else cached0 = f;
            if (f >= n_in) {                                           // the two zero columns behind the spectrogram
                for (int k = tid; k < TS_BINS; k += TS_THREADS) spec[slot][k] = make_float2(0.0f, 0.0f);
                __syncthreads();
                continue;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = tid + TS_THREADS * j;
                TsDf x[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    int m = TS_HOP * f + 2 * n + h - TS_C;             // reflect padding of 1024 on either side (len > 1024)
                    if (m < 0) m = -m;
                    else if (m >= len) m = 2 * (len - 1) - m;
                    const TsDf cs = ts_dc_twiddle(tab, ts_fold(2 * n + h)).re;
                    const TsDf w = ts_df_add(TsDf{0.5f, 0.0f}, TsDf{-0.5f * cs.hi, -0.5f * cs.lo});
                    x[h] = ts_df_mul(TsDf{ts_sample(src, bsrc, al, m), 0.0f}, w);
                }
                ts_dc_store(workd, ts_rev4(n), TsDc{x[0], x[1]});
            }
            ts_fft1024_forward(workd, tab);
            // split step: X[k] = E[k] + W_2048^k O[k], E = (Z[k] + conj Z[1024 - k]) / 2, O = -i (Z[k] - conj Z[1024 - k]) / 2
#pragma unroll
            for (int j = 0; j < 5; ++j) {                              // lane 0 takes bin 1024 as well
                const int k = tid + TS_THREADS * j;
                if (k < TS_BINS) {
                    const TsDc zk = ts_dc_load(workd, k & (TS_C - 1)), zc = ts_dc_load(workd, (TS_C - k) & (TS_C - 1));
                    const TsDc ev = TsDc{ts_df_half(ts_df_add(zk.re, zc.re)), ts_df_half(ts_df_sub(zk.im, zc.im))};
                    const TsDc od = TsDc{ts_df_half(ts_df_add(zk.im, zc.im)), ts_df_half(ts_df_sub(zc.re, zk.re))};
                    const TsDc x = ts_dc_add(ev, ts_dc_mul(od, ts_dc_twiddle(tab, k)));
                    spec[slot][k] = make_float2(x.re.hi, x.im.hi);     // the one rounding of the transform
                }
            }
            __syncthreads();
        }

        // ---- 2. the output column and the phasor update ----
        const float2* __restrict__ d0 = spec[i & 1];
        const float2* __restrict__ d1 = spec[(i + 1) & 1];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int k = tid + TS_THREADS * j;
            if (k < TS_BINS) {
                const float2 z0 = d0[k], z1 = d1[k];
                const float m0 = ts_abs(z0), m1 = ts_abs(z1);
                const float2 u0 = ts_unit(z0, m0), u1 = ts_unit(z1, m1);
                if (t == 0) p[j] = u0;                                 // phase_acc starts at angle(D[:, 0])
                const float mag = (1.0f - af) * m0 + af * m1;
                // irfft reads the real parts of bins 0 and 1024 only
                col[k] = make_float2(mag * p[j].x, (k == 0 || k == TS_C) ? 0.0f : mag * p[j].y);
                const float2 pn = ts_cmul_conj(ts_cmul(p[j], u1), u0);
                const float r = ts_abs(pn);
                p[j] = make_float2(pn.x / r, pn.y / r);
            }
        }
        __syncthreads();

        // ---- 3. irfft(col) w, overlap-add ----
        // Z[k] = E[k] + i O[k], E = X[k] + conj X[1024 - k], O = (X[k] - conj X[1024 - k]) conj(W_2048^k); the halves and the 1 / 1024
        // of the inverse transform are one exact factor at the end
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = tid + TS_THREADS * j;
            const float2 xk = col[k], xc = col[TS_C - k];
            const float2 ev = make_float2(xk.x + xc.x, xk.y - xc.y);
            const float2 od = ts_cmul_conj(make_float2(xk.x - xc.x, xk.y + xc.y), tab[k]);
            work[ts_rev4(k)] = make_float2(ev.x - od.y, ev.y + od.x);
        }
        ts_fft1024<true>(work, tab);
        const int base = TS_HOP * t;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = tid + TS_THREADS * j;
            const float2 z = work[n];
            const float x0 = z.x * (1.0f / TS_N) * ts_hann(tab, 2 * n);
            const float x1 = z.y * (1.0f / TS_N) * ts_hann(tab, 2 * n + 1);
            const int r = (base + 2 * n) & (TS_N - 1);
            if (t == 0 || 2 * n >= TS_N - TS_HOP) {                    // the quarter no earlier frame reaches: the ring starts over
                ring[r] = x0, ring[r + 1] = x1;
            } else {
                ring[r] += x0, ring[r + 1] += x1;
            }
        }
        __syncthreads();
        retire(base, TS_HOP);
        __syncthreads();
    }
    retire(TS_HOP * n_used, TS_N - TS_HOP);                            // what the last frame leaves in the ring
    for (int o = TS_HOP * (n_used - 1) + TS_C + tid; o < out_len; o += TS_THREADS) dst[o] = 0.0f;   // fix_length's zero tail
}

}  // namespace

extern "C" {

int howl_timestretch_clips(const float* bank, long bank_ld, long bank_floats, const float* bg, long bg_ld, long bg_floats,
                           const HowlStretchClip* clips_host, const HowlStretchClip* clips_dev, int B, float* out, long out_floats,
                           unsigned flags, hipStream_t stream) {
    HOWL_REQUIRE(bank && clips_host && clips_dev && out, "howl_timestretch_clips: null pointer");
    HOWL_REQUIRE(B >= 1 && B <= HOWL_TIMESTRETCH_MAX_CLIPS, "howl_timestretch_clips: B=%d clips unsupported (1..%d)", B,
                 HOWL_TIMESTRETCH_MAX_CLIPS);
    HOWL_REQUIRE(bank_ld >= 0 && bank_floats >= 0 && bg_ld >= 0 && out_floats >= 0 && (bg == nullptr || bg_floats >= 0),
                 "howl_timestretch_clips: negative size or stride");
    HOWL_REQUIRE((flags & ~HOWL_TIMESTRETCH_NO_COPY) == 0, "howl_timestretch_clips: flags=0x%x unsupported", flags);
    for (int b = 0; b < B; ++b) {
        const HowlStretchClip& c = clips_host[b];
        HOWL_REQUIRE(c.rate == 1.0 || (c.rate >= HOWL_TIMESTRETCH_MIN_RATE && c.rate <= HOWL_TIMESTRETCH_MAX_RATE),
                     "howl_timestretch_clips: clip %d: rate=%g unsupported (1.0, or %g..%g)", b, c.rate, HOWL_TIMESTRETCH_MIN_RATE,
                     HOWL_TIMESTRETCH_MAX_RATE);
        HOWL_REQUIRE(c.len >= 1 && c.len <= HOWL_TIMESTRETCH_MAX_SAMPLES, "howl_timestretch_clips: clip %d: len=%d samples unsupported (1..%d)",
                     b, c.len, HOWL_TIMESTRETCH_MAX_SAMPLES);
        HOWL_REQUIRE(c.rate == 1.0 || c.len >= HOWL_TIMESTRETCH_MIN_SAMPLES,
                     "howl_timestretch_clips: clip %d: len=%d samples with rate=%g unsupported (a clip under %d samples keeps rate 1.0)", b,
                     c.len, c.rate, HOWL_TIMESTRETCH_MIN_SAMPLES);
        HOWL_REQUIRE(!(flags & HOWL_TIMESTRETCH_NO_COPY) || c.len >= HOWL_TIMESTRETCH_MIN_SAMPLES,
                     "howl_timestretch_clips: clip %d: len=%d samples through the transform unsupported (>= %d)", b, c.len,
                     HOWL_TIMESTRETCH_MIN_SAMPLES);
        const long want_len = (long)nearbyint((double)c.len / c.rate);                     // Python's round: half to even
        const long want_n = (long)ceil((double)(1 + c.len / 512) / c.rate);                // len(np.arange(0, n_in, rate))
        HOWL_REQUIRE(c.out_len == want_len && c.n_out == want_n,
                     "howl_timestretch_clips: clip %d: out_len=%d, n_out=%d; len=%d at rate=%.17g gives %ld and %ld", b, c.out_len, c.n_out,
                     c.len, c.rate, want_len, want_n);
        HOWL_REQUIRE(c.src_row >= 0 && (c.src_row == 0 || bank_ld <= bank_floats / c.src_row) &&
                         c.src_row * bank_ld + c.len <= bank_floats,
                     "howl_timestretch_clips: clip %d: source row %lld, %d samples, outside the bank of %ld floats", b, c.src_row, c.len,
                     bank_floats);
        HOWL_REQUIRE(c.dst_off >= 0 && c.dst_off <= out_floats - c.out_len,
                     "howl_timestretch_clips: clip %d: output [%lld, +%d) outside the destination of %ld floats", b, c.dst_off, c.out_len,
                     out_floats);
        if (c.alpha != 0.0f) {
            HOWL_REQUIRE(bg != nullptr, "howl_timestretch_clips: clip %d: alpha=%g without a background bank", b, c.alpha);
            HOWL_REQUIRE(c.bg_idx >= 0 && c.bg_off >= 0 && (c.bg_idx == 0 || bg_ld <= bg_floats / c.bg_idx) &&
                             (long)c.bg_idx * bg_ld + c.bg_off + c.len <= bg_floats,
                         "howl_timestretch_clips: clip %d: background row %d offset %d, %d samples, outside the bank of %ld floats", b,
                         c.bg_idx, c.bg_off, c.len, bg_floats);
        }
    }
    TsArgs a;
    a.bank = bank, a.bank_ld = bank_ld, a.bg = bg, a.bg_ld = bg_ld, a.clips = clips_dev, a.out = out, a.flags = flags;
    hipLaunchKernelGGL(timestretch_kernel, dim3((unsigned)B), dim3(TS_THREADS), 0, stream, a);
    HOWL_CHECK_LAUNCH("howl_timestretch_clips");
    return HOWL_OK;
}

}  // extern "C"
