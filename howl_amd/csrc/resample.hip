// Clips of any sample rate (include/howl_hip_resample.h): channel mean + polyphase Kaiser-windowed-sinc FIR over B ragged clips in
// ONE launch.  A 256-thread workgroup per (clip, tile of 256 consecutive outputs):
//   1. the tile's input span -- floor(n0 D / U) + j_lo .. floor((n0 + 255) D / U) + j_lo + taps -- is staged once into LDS; the
//      int16 -> float conversion and the channel mean happen here, frames outside the clip become 0 (the mono float clip never
//      exists in memory);
//   2. every lane owns ONE output and walks its phase's whole bank row against the span, four taps (one 16-byte read of the row)
//      per step into four partial sums, folded (a0 + a1) + (a2 + a3): a fixed order per output, so a clip's bits depend neither
//      on its neighbours, nor on dst_off, nor on where a tile boundary falls.
// Where the bank row comes from:
//   U <= 2 (48, 32, 96, 8, 24 kHz -> 16 kHz): the whole bank is copied into LDS and lanes are dealt so that a wave has ONE phase
//          (thread t: phase group t / (256 / U), output n0 + (t % (256 / U)) U + group): the row read is an LDS broadcast;
//   U >  2 (44.1, 22.05, 11.025 kHz): the bank (up to ~330 KB) stays in global memory, L2-resident; lane t owns output n0 + t, so
//          the lanes of a wave read 64 different rows, each lane streaming its own row front to back.
#include <math.h>

#include "howl_common.hip.h"
#include "../../include/howl_hip_resample.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_TILE = 256;          // outputs per workgroup
constexpr double RS_ROLLOFF = 0.9475937167399596;
constexpr double RS_BETA = 14.769656459379492;

struct RsArgs {
    const void* src;
    const float* bank;
    const HowlResampleClip* clips;
    float* out;
    int channels, up, down, taps, j_lo;
};

// ---- host: the plan and the bank ----
long long rs_gcd(long long a, long long b) {
    while (b) {
        const long long t = a % b;
        a = b, b = t;
    }
    return a;
}

// modified Bessel function of the first kind, order 0: sum_k ((x/2)^2k / (k!)^2), all terms positive (x <= beta here)
double rs_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

double rs_h(double t) {
    const double u = t / HOWL_RESAMPLE_ZEROS;
    const double w = rs_i0(RS_BETA * sqrt(fmax(0.0, 1.0 - u * u))) / rs_i0(RS_BETA);
    const double x = M_PI * RS_ROLLOFF * t;
    return RS_ROLLOFF * (x == 0.0 ? 1.0 : sin(x) / x) * w;
}

bool rs_make_plan(int sr_in, int sr_out, HowlResamplePlan* p) {
    if (sr_in < HOWL_RESAMPLE_MIN_RATE || sr_in > HOWL_RESAMPLE_MAX_RATE || sr_out < HOWL_RESAMPLE_MIN_RATE ||
        sr_out > HOWL_RESAMPLE_MAX_RATE)
        return false;
    const long long g = rs_gcd(sr_in, sr_out);
    const long long U = sr_out / g, D = sr_in / g;
    if (U > HOWL_RESAMPLE_MAX_UP || D > HOWL_RESAMPLE_MAX_DECIMATION * U) return false;
    p->sr_in = sr_in, p->sr_out = sr_out, p->up = (int)U, p->down = (int)D, p->reserved = 0;
    if (U == 1 && D == 1) {
        p->j_lo = p->j_hi = 0, p->taps = 4, p->s = 1.0;
        return true;
    }
    const long long W = HOWL_RESAMPLE_ZEROS * (U > D ? U : D);        // |p - j U| < W  <=>  |t| < Z
    p->j_lo = (int)-((W - 1) / U);                                    // phase 0 reaches furthest back
    p->j_hi = (int)((W + U - 2) / U);                                 // phase U - 1 furthest ahead
    p->taps = (p->j_hi - p->j_lo + 1 + 3) & ~3;
    p->s = U < D ? (double)U / (double)D : 1.0;
    return true;
}

bool rs_plan_ok(const HowlResamplePlan* p) {
    HowlResamplePlan q;
    if (p == nullptr || !rs_make_plan(p->sr_in, p->sr_out, &q)) return false;
    return q.up == p->up && q.down == p->down && q.taps == p->taps && q.j_lo == p->j_lo && q.j_hi == p->j_hi && q.s == p->s;
}

inline long long rs_full_len(const HowlResamplePlan* p, long long len) { return (len * p->up + p->down - 1) / p->down; }

// ---- device ----
template <int FORMAT>
__device__ __forceinline__ float rs_frame(const void* __restrict__ src, long long frame, int channels) {
    float sum = 0.0f;
    if (FORMAT == HOWL_RESAMPLE_I16) {
        const short* __restrict__ v = static_cast<const short*>(src) + frame * channels;
        sum = (float)v[0] * (1.0f / 32768.0f);
        for (int ch = 1; ch < channels; ++ch) sum += (float)v[ch] * (1.0f / 32768.0f);
    } else {
        const float* __restrict__ v = static_cast<const float*>(src) + frame * channels;
        sum = v[0];
        for (int ch = 1; ch < channels; ++ch) sum += v[ch];
    }
    return channels == 1 ? sum : sum / (float)channels;
}

template <int FORMAT, bool ROWS_IN_LDS>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(RsArgs a) {
    HIP_DYNAMIC_SHARED(float, lds)
    const int tid = threadIdx.x;
    const HowlResampleClip c = a.clips[blockIdx.y];
    const long long n0 = (long long)blockIdx.x * RS_TILE;
    if (n0 >= c.out_len) return;                                      // the grid is as wide as the longest clip of the batch
    const int U = a.up, D = a.down, taps = a.taps;
    const long long base0 = n0 * D / U;
    const int span = (int)((n0 + RS_TILE - 1) * D / U - base0) + taps;
    float* const xs = lds;                                            // span floats
    float* const rows = lds + ((span + 3) & ~3);                      // ROWS_IN_LDS: the bank, U * taps floats (16-byte aligned)

    const long long k0 = base0 + a.j_lo;                              // input frame of xs[0]
    for (int f = tid; f < span; f += RS_THREADS) {
        const long long k = k0 + f;
        xs[f] = (k >= 0 && k < c.len) ? rs_frame<FORMAT>(a.src, c.src_off + k, a.channels) : 0.0f;
    }
    if (ROWS_IN_LDS) {
        const float4* __restrict__ b4 = reinterpret_cast<const float4*>(a.bank);
        for (int q = tid; q < U * taps / 4; q += RS_THREADS) reinterpret_cast<float4*>(rows)[q] = b4[q];
    }
    __syncthreads();

    long long n;
    if (ROWS_IN_LDS) {
        const int per = RS_THREADS / U;                               // U is 1 or 2: a wave holds one phase
        n = n0 + (long long)(tid % per) * U + tid / per;
    } else {
        n = n0 + tid;
    }
    if (n >= c.out_len) return;
    const long long nd = n * D;
    const int p = (int)(nd % U);
    const float* __restrict__ x = xs + (int)(nd / U - base0);
    const float4* __restrict__ row = reinterpret_cast<const float4*>((ROWS_IN_LDS ? rows : a.bank) + (long)p * taps);
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    for (int i = 0; i < taps / 4; ++i) {
        const float4 w = row[i];
        a0 = fmaf(w.x, x[4 * i], a0);
        a1 = fmaf(w.y, x[4 * i + 1], a1);
        a2 = fmaf(w.z, x[4 * i + 2], a2);
        a3 = fmaf(w.w, x[4 * i + 3], a3);
    }
    a.out[c.dst_off + n] = (a0 + a1) + (a2 + a3);
}

}  // namespace

extern "C" {

int howl_resample_plan(int sr_in, int sr_out, HowlResamplePlan* plan) {
    HOWL_REQUIRE(plan != nullptr, "howl_resample_plan: null pointer");
    HOWL_REQUIRE(rs_make_plan(sr_in, sr_out, plan),
                 "howl_resample_plan: %d Hz -> %d Hz unsupported (rates %d..%d, reduced up factor <= %d, decimation <= %d)", sr_in, sr_out,
                 HOWL_RESAMPLE_MIN_RATE, HOWL_RESAMPLE_MAX_RATE, HOWL_RESAMPLE_MAX_UP, HOWL_RESAMPLE_MAX_DECIMATION);
    return HOWL_OK;
}

size_t howl_resample_bank_floats(const HowlResamplePlan* plan) { return rs_plan_ok(plan) ? (size_t)plan->up * (size_t)plan->taps : 0; }

int howl_resample_bank(const HowlResamplePlan* plan, float* bank_host) {
    HOWL_REQUIRE(plan != nullptr && bank_host != nullptr, "howl_resample_bank: null pointer");
    HOWL_REQUIRE(rs_plan_ok(plan), "howl_resample_bank: the plan is not howl_resample_plan's for %d Hz -> %d Hz", plan->sr_in, plan->sr_out);
    const long long U = plan->up, D = plan->down, M = U > D ? U : D;
    if (U == 1 && D == 1) {
        bank_host[0] = 1.0f, bank_host[1] = bank_host[2] = bank_host[3] = 0.0f;
        return HOWL_OK;
    }
    for (long long p = 0; p < U; ++p) {
        for (int i = 0; i < plan->taps; ++i) {
            const long long num = p - (plan->j_lo + (long long)i) * U;                 // t = num / M
            const bool inside = (num < 0 ? -num : num) < HOWL_RESAMPLE_ZEROS * M;
            bank_host[p * plan->taps + i] = inside ? (float)(plan->s * rs_h((double)num / (double)M)) : 0.0f;
        }
    }
    return HOWL_OK;
}

size_t howl_resample_out_len(const HowlResamplePlan* plan, long len) {
    return (len >= 0 && rs_plan_ok(plan)) ? (size_t)rs_full_len(plan, len) : 0;
}

int howl_resample_clips(const void* src, long src_elems, int format, int channels, const float* bank_dev, long bank_floats,
                        const HowlResamplePlan* plan, const HowlResampleClip* clips_host, const HowlResampleClip* clips_dev, int B,
                        float* out, long out_floats, hipStream_t stream) {
    HOWL_REQUIRE(src && bank_dev && plan && clips_host && clips_dev && out, "howl_resample_clips: null pointer");
    HOWL_REQUIRE(rs_plan_ok(plan), "howl_resample_clips: the plan is not howl_resample_plan's for %d Hz -> %d Hz", plan->sr_in, plan->sr_out);
    HOWL_REQUIRE(bank_floats == (long)plan->up * plan->taps, "howl_resample_clips: bank of %ld floats; the plan for %d Hz -> %d Hz has %d x %d",
                 bank_floats, plan->sr_in, plan->sr_out, plan->up, plan->taps);
    HOWL_REQUIRE(format == HOWL_RESAMPLE_F32 || format == HOWL_RESAMPLE_I16, "howl_resample_clips: format=%d unsupported (0: float32, 1: int16)",
                 format);
    HOWL_REQUIRE(channels >= 1 && channels <= HOWL_RESAMPLE_MAX_CHANNELS, "howl_resample_clips: channels=%d unsupported (1..%d)", channels,
                 HOWL_RESAMPLE_MAX_CHANNELS);
    HOWL_REQUIRE(B >= 1 && B <= HOWL_RESAMPLE_MAX_CLIPS, "howl_resample_clips: B=%d clips unsupported (1..%d)", B, HOWL_RESAMPLE_MAX_CLIPS);
    HOWL_REQUIRE(src_elems >= 0 && out_floats >= 0, "howl_resample_clips: negative size");
    const long src_frames = src_elems / channels;
    int longest = 0;
    for (int b = 0; b < B; ++b) {
        const HowlResampleClip& c = clips_host[b];
        HOWL_REQUIRE(c.len >= 1 && c.len <= HOWL_RESAMPLE_MAX_FRAMES, "howl_resample_clips: clip %d: len=%d frames unsupported (1..%d)", b, c.len,
                     HOWL_RESAMPLE_MAX_FRAMES);
        const long long full = rs_full_len(plan, c.len);
        HOWL_REQUIRE(c.out_len >= 0 && c.out_len <= full, "howl_resample_clips: clip %d: out_len=%d; len=%d at %d/%d gives at most %lld", b,
                     c.out_len, c.len, plan->up, plan->down, full);
        HOWL_REQUIRE(c.src_off >= 0 && c.src_off <= src_frames - c.len,
                     "howl_resample_clips: clip %d: source frames [%lld, +%d) outside the buffer of %ld frames", b, c.src_off, c.len, src_frames);
        HOWL_REQUIRE(c.dst_off >= 0 && c.dst_off <= out_floats - c.out_len,
                     "howl_resample_clips: clip %d: output [%lld, +%d) outside the destination of %ld floats", b, c.dst_off, c.out_len, out_floats);
        if (c.out_len > longest) longest = c.out_len;
    }
    if (longest == 0) return HOWL_OK;
    RsArgs a;
    a.src = src, a.bank = bank_dev, a.clips = clips_dev, a.out = out;
    a.channels = channels, a.up = plan->up, a.down = plan->down, a.taps = plan->taps, a.j_lo = plan->j_lo;
    const bool in_lds = plan->up <= 2;
    const long span_max = (long)(RS_TILE - 1) * plan->down / plan->up + 1 + plan->taps;
    const size_t lds = (size_t)(((span_max + 3) & ~3L) + (in_lds ? (long)plan->up * plan->taps : 0)) * sizeof(float);
    const dim3 grid((unsigned)((longest + RS_TILE - 1) / RS_TILE), (unsigned)B);
    if (format == HOWL_RESAMPLE_I16) {
        if (in_lds) hipLaunchKernelGGL((resample_kernel<HOWL_RESAMPLE_I16, true>), grid, dim3(RS_THREADS), lds, stream, a);
        else hipLaunchKernelGGL((resample_kernel<HOWL_RESAMPLE_I16, false>), grid, dim3(RS_THREADS), lds, stream, a);
    } else {
        if (in_lds) hipLaunchKernelGGL((resample_kernel<HOWL_RESAMPLE_F32, true>), grid, dim3(RS_THREADS), lds, stream, a);
        else hipLaunchKernelGGL((resample_kernel<HOWL_RESAMPLE_F32, false>), grid, dim3(RS_THREADS), lds, stream, a);
    }
    HOWL_CHECK_LAUNCH("howl_resample_clips");
    return HOWL_OK;
}

}  // extern "C"
