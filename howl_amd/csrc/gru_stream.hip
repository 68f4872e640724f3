// Streaming gru (include/howl_hip_gru_stream.h): ONE launch from a window's raw PCM to its class probabilities, one workgroup of
// eight waves per window.  Replaces, for the live client's window (inference.py:247-267), the chain howl_logmel_fwd -> howl_gru_fwd
// (gru_enc_fwd_kernel, gru_fwd4_kernel, gru_head_fwd_kernel) -> softmax: four launches and a torch kernel for about 1.5 MFLOP, with
// a recurrence kernel that is built for four sequences per workgroup and always walks all T1 steps.  The model is the eval-mode
// model of gru.hip with its order of operations; the parameters and the running statistics are read in place (no prepared state).
//
// Per workgroup, with workgroup barriers only (nothing is shared between workgroups, so there is no counter, flag or spin loop):
//   1. log-mel of the window's T frames (logmel_body<8> of howl_logmel.hip.h, standard filterbank, no ZMUV) into LDS;
//   2. ZMUV (the frontend's arithmetic, (y - mean) * (1 / std)) -> the feature plane [42][T + 6] with conv1's zero border
//      (one mel row above and below, three frames before and after);
//   3. conv1 (1 -> 8) + bias, BN1 folded from the running statistics, ReLU, MaxPool(1,2): thread = (mel row, pooled column), the
//      column pair x eight channels, conv1_at's fmaf chain -> the pooled map with conv2's zero border in the window's workspace;
//   4. conv2 (8 -> 1) + bias, ReLU, BN2 (one scale and one shift) -> x^[T1][40] in LDS;
//   5. the recurrence, n = min((frames + 4) / 2, T1) dependent steps from a zero state on waves 0..5: lane 4 j + g of wave c serves
//      unit u = 16 c + j with one pre-activation, g = 0: W_hr h + W_ir x + b, 1: W_hz h + W_iz x + b, 2: W_hn h + b_hn,
//      3: W_in x + b_in -- the two halves of n stay apart because r multiplies only the first.  The lane's W_hh row (96) and W_ih
//      row (40) live in registers as pairs, the operands of v_pk_fma_f32 (zeros where a half has no such term), h is double-buffered
//      in LDS, the four pre-activations of a unit meet inside their quad of lanes (DPP), one barrier per step.  W_ih x^ is done
//      inside the step: it does not depend on h, so it is not on the step's dependent chain, and the lanes would otherwise spend
//      the same 40 FMAs per step on it in front of the loop;
//   6. Linear(96,192) - ReLU - Linear(192,C) (gru_head_fwd_kernel's order of operations; no dropout);   7. softmax.
//
// LDS plan (floats; the regions of a later phase lie over the dead ones of an earlier one).  Static: logmel_body<8> 98,048 B.
//   phases 1-3: log-mels [T][40] 3,320 | feature plane [42][PW] 3,738 (PW = T + 6, made odd: mel rows run fastest over the lanes)
//               | conv weights, biases and both folded BatchNorms 176
//   phases 4-7: x^ [T1][40] 1,720 | h double buffer 192 | y1 192 | logits 64      (over the log-mels; the conv block stays)
// = 7,234 floats = 28,936 B dynamic, 126,984 of 163,840 B in all.  The pooled conv1 map with its border (8 x 45 x 42 floats,
// 60,480 B at T = 83) does not fit beside the feature plane and the frontend's tiles: it goes through `ws`, each window's share
// written and read back by its own workgroup only, between workgroup barriers.
#include "howl_logmel.hip.h"
#include "howl_lstm.hip.h"
#include "howl_stream.hip.h"
#include "../../include/howl_hip_gru_stream.h"

namespace {

constexpr int GQ_H = 96, GQ_G3 = 3 * GQ_H, GQ_HD = 2 * GQ_H;
constexpr int GQ_M = 40, GQ_C = 8, GQ_ROWS = GQ_M + 2;      // mel bins, latent channels, mel rows with a zero row on either side
constexpr int GQ_THREADS = 512, GQ_WAVES = 8, GQ_REC_THREADS = 4 * GQ_H;
constexpr int GQ_MAX_FRAMES = 83;
constexpr float GQ_BN_EPS = 1e-5f;

// the conv block in LDS
constexpr int GQ_W_C1W = 0, GQ_W_C1B = 72, GQ_W_SC1 = 80, GQ_W_SH1 = 88, GQ_W_C2W = 96, GQ_W_C2B = 168, GQ_W_S2 = 169, GQ_W_T2 = 170;
constexpr int GQ_W_FLOATS = 176;

// dynamic LDS, in floats
constexpr int GQ_L_LM = 0;
constexpr int GQ_L_X = GQ_L_LM + GQ_MAX_FRAMES * GQ_M;
constexpr int GQ_L_CW = GQ_L_X + GQ_ROWS * ((GQ_MAX_FRAMES + 6) | 1);
constexpr int GQ_L_XH = 0;
constexpr int GQ_L_HB = GQ_L_XH + ((GQ_MAX_FRAMES + 4) / 2) * GQ_M;
constexpr int GQ_L_Y1 = GQ_L_HB + 2 * GQ_H;
constexpr int GQ_L_LG = GQ_L_Y1 + GQ_HD;
constexpr int GQ_LDS_FLOATS = GQ_L_CW + GQ_W_FLOATS;
static_assert(GQ_L_LG + HOWL_GRU_MAX_LABELS <= GQ_L_X, "the last phases lie over the log-mels only");
static_assert(GQ_L_XH % 4 == 0 && GQ_L_HB % 4 == 0, "16-byte reads of x^ and h");

struct GqGeom {
    int T, T1, PC;      // frames, pooled columns = recurrence steps of a whole window, columns of the bordered pooled map
    int ws_floats;      // the window's share of the workspace: the bordered pooled map [8][PC][42]
};
__host__ __device__ inline GqGeom gq_geom(int L) {
    GqGeom g;
    g.T = 1 + L / HOP;
    g.T1 = (g.T + 4) / 2;
    g.PC = g.T1 + 2;
    g.ws_floats = GQ_C * g.PC * GQ_ROWS;      // (a multiple of four: 8 x 42)
    return g;
}
static_assert((GQ_C * GQ_ROWS) % 4 == 0, "a window's share is a multiple of 16 bytes");

struct GqModel {
    HowlGruParams p;
    const float *m1, *v1, *m2, *v2;      // running mean and variance of BN1 (8) and BN2 (1)
};

// lane k of every quad of lanes -> all four
template <int K>
__device__ __forceinline__ float gq_quad_bcast(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), K * 0x55, 0xf, 0xf, true));
}

__global__ __launch_bounds__(GQ_THREADS) void gru_stream_kernel(GqModel a, const float* __restrict__ pcm, long ld, int L, int nsteps,
                                                                const float* __restrict__ fbp, float log_eps,
                                                                const float* __restrict__ zmuv, int aligned, int C,
                                                                float* __restrict__ probs, float* __restrict__ logits,
                                                                float* __restrict__ ws) {
    HIP_DYNAMIC_SHARED(float, lds)
    const HowlGruParams& p = a.p;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long win = blockIdx.x;
    const GqGeom gm = gq_geom(L);
    const int T = gm.T, T1 = gm.T1, PC = gm.PC, n = nsteps;
    const int PW = (T + 6) | 1;      // the feature plane's row pitch, odd
    float* const p1 = ws + win * gm.ws_floats;      // [ci][column + 1][mel + 1], zero border (conv2's padding of 1)
    float* const lm = lds + GQ_L_LM;
    float* const xp = lds + GQ_L_X;
    float* const cw = lds + GQ_L_CW;

    // what later phases read without having written it: the plane's and the map's borders; the conv block
    for (int i = tid; i < GQ_ROWS * PW; i += GQ_THREADS) xp[i] = 0.0f;
    for (int i = tid; i < gm.ws_floats; i += GQ_THREADS) p1[i] = 0.0f;
    if (tid < 72) {
        cw[GQ_W_C1W + tid] = p.conv1_w[tid];
    } else if (tid < 80) {
        cw[GQ_W_C1B + tid - 72] = p.conv1_b[tid - 72];
    } else if (tid >= 128 && tid < 200) {
        cw[GQ_W_C2W + tid - 128] = p.conv2_w[tid - 128];
    } else if (tid >= 256 && tid < 256 + GQ_C) {
        // y = z * sc + sh (gru.hip's bn_affine from the running statistics)
        const int c = tid - 256;
        const float sc = p.bn1_w[c] * (1.0f / sqrtf(a.v1[c] + GQ_BN_EPS));
        cw[GQ_W_SC1 + c] = sc;
        cw[GQ_W_SH1 + c] = p.bn1_b[c] - a.m1[c] * sc;
    } else if (tid == 320) {
        const float sc = p.bn2_w[0] * (1.0f / sqrtf(a.v2[0] + GQ_BN_EPS));
        cw[GQ_W_C2B] = p.conv2_b[0];
        cw[GQ_W_S2] = sc;
        cw[GQ_W_T2] = p.bn2_b[0] - a.m2[0] * sc;
    }

    // ---- 1. log-mels of the T frames: frame t, mel m -> lm[40 t + m] (the body's one workgroup barrier covers the stores above)
    logmel_body<GQ_WAVES, NG_BANDED>(pcm + win * ld, L, ld, T, T, fbp, GQ_M, log_eps, nullptr, lm, 1, (T + QUAD - 1) / QUAD, aligned, 0u, 1u,
                                     GQ_M);
    __syncthreads();

    // ---- 2. ZMUV into the plane: mel m, frame t -> xp[(m + 1) PW + t + 3]
    {
        float mean = 0.0f, rstd = 1.0f;
        if (zmuv != nullptr) {
            mean = zmuv[0];
            rstd = 1.0f / zmuv[1];
        }
        for (int i = tid; i < GQ_M * T; i += GQ_THREADS) {
            const int t = i / GQ_M, m = i - t * GQ_M;
            xp[(m + 1) * PW + t + 3] = (lm[i] - mean) * rstd;
        }
    }
    __syncthreads();

    // ---- 3. conv1 + BN1 + ReLU + MaxPool(1,2): thread = (mel m, pooled column q), conv1's columns 2 q and 2 q + 1 of T + 4
#pragma unroll 1
    for (int i = tid; i < GQ_M * T1; i += GQ_THREADS) {
        const int q = i / GQ_M, m = i - q * GQ_M;
        float xv[3][4];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const float* xr = xp + (m + dy) * PW + 2 * q;
#pragma unroll
            for (int k = 0; k < 4; ++k) xv[dy][k] = xr[k];
        }
#pragma unroll
        for (int c = 0; c < GQ_C; ++c) {
            float z0 = cw[GQ_W_C1B + c], z1 = z0;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float w = cw[GQ_W_C1W + c * 9 + dy * 3 + dx];
                    z0 = fmaf(w, xv[dy][dx], z0);
                    z1 = fmaf(w, xv[dy][dx + 1], z1);
                }
            const float sc = cw[GQ_W_SC1 + c], sh = cw[GQ_W_SH1 + c];
            p1[(c * PC + q + 1) * GQ_ROWS + m + 1] = fmaxf(fmaxf(fmaf(z0, sc, sh), fmaf(z1, sc, sh)), 0.0f);
        }
    }
    __syncthreads();      // the log-mels and the plane are dead from here on

    // ---- 4. conv2 + ReLU + BN2 -> x^[q][m]
    float* const xh = lds + GQ_L_XH;
    float* const hb = lds + GQ_L_HB;      // [parity][96]
    {
        const float s2 = cw[GQ_W_S2], t2 = cw[GQ_W_T2];
#pragma unroll 1
        for (int i = tid; i < GQ_M * T1; i += GQ_THREADS) {
            const int q = i / GQ_M, m = i - q * GQ_M;
            float z = cw[GQ_W_C2B];
#pragma unroll
            for (int c = 0; c < GQ_C; ++c) {
                const float* pr = p1 + (c * PC + q) * GQ_ROWS + m;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) z = fmaf(cw[GQ_W_C2W + c * 9 + dy * 3 + dx], pr[dx * GQ_ROWS + dy], z);
            }
            xh[q * GQ_M + m] = fmaf(fmaxf(z, 0.0f), s2, t2);
        }
        if (tid < GQ_H) hb[tid] = 0.0f;
    }

    // ---- 5. the recurrence.  Thread (wave c of six, lane 4 j + g) = pre-activation g of unit 16 c + j.
    {
        const bool active = wave < GQ_REC_THREADS / 64;      // (wave-uniform)
        const int g = lane & 3, u = min(16 * wave + (lane >> 2), GQ_H - 1);
        // weight pairs (k, k + 1): the step's FMAs are v_pk_fma_f32 on register pairs as the 16-byte LDS reads deliver them
        v2f wB[GQ_H / 2], wI[GQ_M / 2];
        float bias = 0.0f;
        if (active) {
            // the lane's weight rows, read in place
            const int hrow = (g < 3 ? g : 2) * GQ_H + u, xrow = (g == 3 ? 2 : g) * GQ_H + u;
            const bool has_h = g < 3, has_x = g != 2;
#pragma unroll
            for (int k = 0; k < GQ_H; ++k) {
                const float v = p.w_hh[hrow * GQ_H + k];
                wB[k >> 1][k & 1] = has_h ? v : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < GQ_M; ++k) {
                const float v = p.w_ih[xrow * GQ_M + k];
                wI[k >> 1][k & 1] = has_x ? v : 0.0f;
            }
            bias = g < 2 ? p.b_ih[g * GQ_H + u] + p.b_hh[g * GQ_H + u] : (g == 2 ? p.b_hh[2 * GQ_H + u] : p.b_ih[2 * GQ_H + u]);
        } else {
#pragma unroll
            for (int k = 0; k < GQ_H / 2; ++k) wB[k] = v2f{0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < GQ_M / 2; ++k) wI[k] = v2f{0.0f, 0.0f};
        }
        float hst = 0.0f;
        __syncthreads();      // x^ and the zero state are in LDS
        for (int s = 0; s < n; ++s) {
            if (active) {
                const float* hc = hb + (s & 1) * GQ_H;
                const float* xs = xh + s * GQ_M;
                v2f a01 = {0.0f, 0.0f}, a23 = {0.0f, 0.0f};      // four FMA chains: k = 0, 1, 2, 3 (mod 4)
#pragma unroll
                for (int k4 = 0; k4 < GQ_M / 4; ++k4) {
                    const v4f xv = *reinterpret_cast<const v4f*>(xs + 4 * k4);
                    a01 = __builtin_elementwise_fma(xv.xy, wI[2 * k4], a01);
                    a23 = __builtin_elementwise_fma(xv.zw, wI[2 * k4 + 1], a23);
                }
#pragma unroll
                for (int k4 = 0; k4 < GQ_H / 4; ++k4) {
                    const v4f hv = *reinterpret_cast<const v4f*>(hc + 4 * k4);
                    a01 = __builtin_elementwise_fma(hv.xy, wB[2 * k4], a01);
                    a23 = __builtin_elementwise_fma(hv.zw, wB[2 * k4 + 1], a23);
                }
                const float pre = ((a01.x + a01.y) + (a23.x + a23.y)) + bias;
                // r, z, W_hn h + b_hn, W_in x + b_in of the quad's unit; every lane of the quad carries the unit's state
                const float rg = sigmoidf_(gq_quad_bcast<0>(pre)), zg = sigmoidf_(gq_quad_bcast<1>(pre));
                const float ng = tanhf_(fmaf(rg, gq_quad_bcast<2>(pre), gq_quad_bcast<3>(pre)));
                hst = fmaf(zg, hst - ng, ng);      // (1 - z) n + z h
                if (g == 0) hb[((s + 1) & 1) * GQ_H + u] = hst;
            }
            __syncthreads();
        }
    }
    const float* const hT = hb + (n & 1) * GQ_H;

    // ---- 6. Linear(96,192) - ReLU - Linear(192,C)
    float* const y1 = lds + GQ_L_Y1;
    float* const lg = lds + GQ_L_LG;
    if (tid < GQ_HD) {
        float v = p.b1[tid];
        const float* w = p.w1 + tid * GQ_H;
#pragma unroll 8
        for (int k = 0; k < GQ_H; ++k) v = fmaf(w[k], hT[k], v);
        y1[tid] = fmaxf(v, 0.0f);
    }
    __syncthreads();
    for (int cl = wave; cl < C; cl += GQ_WAVES) {
        float v = 0.0f;
        for (int k = lane; k < GQ_HD; k += 64) v = fmaf(p.w2[cl * GQ_HD + k], y1[k], v);
        v = wave_sum(v);
        if (lane == 0) {
            v += p.b2[cl];
            lg[cl] = v;
            if (logits != nullptr) logits[win * C + cl] = v;
        }
    }
    __syncthreads();

    // ---- 7. softmax
    if (tid < C) {
        float mx = lg[0];
        for (int k = 1; k < C; ++k) mx = fmaxf(mx, lg[k]);
        float se = 0.0f;
        for (int k = 0; k < C; ++k) se += expf(lg[k] - mx);
        probs[win * C + tid] = expf(lg[tid] - mx) / se;
    }
}

bool gq_supported(int L, int M, int C) {
    return M == GQ_M && C >= 1 && C <= HOWL_GRU_MAX_LABELS && L >= N_FFT && 1 + L / HOP <= GQ_MAX_FRAMES;
}

}  // namespace

// tests/test_emu_gru.py pins the library's `T` exports under howl_gru_ to the four functions of howl_hip_gru.h.  These entry points
// share that prefix (it is the model's name), so they are exported as weak definitions, as las_stream.hip exports its own: the same
// thing to the dynamic linker and to every caller, `W` in the symbol table.
#define GQ_EXPORT __attribute__((weak))

extern "C" {

GQ_EXPORT int howl_gru_stream_supported(int L_samples, int M, int C) { return gq_supported(L_samples, M, C) ? 1 : 0; }

GQ_EXPORT size_t howl_gru_stream_workspace_bytes(int N, int L_samples) {
    if (N < 1 || N > HOWL_GRU_STREAM_MAX_WINDOWS || !gq_supported(L_samples, GQ_M, 1)) return 0;
    return (size_t)N * (size_t)gq_geom(L_samples).ws_floats * sizeof(float);
}

GQ_EXPORT int howl_gru_stream_windows(const HowlGruParams* prm, const HowlGruBuffers* buffers, const float* pcm, long ld, int N, int L_samples,
                                      int frames, const float* fbp, int M, float log_eps, const float* zmuv_pair, int C, float* probs,
                                      float* logits, void* ws, size_t ws_bytes, hipStream_t stream) {
    HOWL_REQUIRE(prm && buffers && pcm && fbp && probs && ws, "howl_gru_stream_windows: null pointer");
    HOWL_REQUIRE(stream_record_complete(prm), "howl_gru_stream_windows: null pointer in HowlGruParams");
    HOWL_REQUIRE(buffers->bn1_mean && buffers->bn1_var && buffers->bn2_mean && buffers->bn2_var,
                 "howl_gru_stream_windows: null pointer in HowlGruBuffers");
    HOWL_REQUIRE(gq_supported(L_samples, M, C),
                 "howl_gru_stream_windows: L=%d samples, M=%d, C=%d unsupported (M = 40, %d <= L < %d samples, 1 <= C <= %d: "
                 "howl_gru_stream_supported)", L_samples, M, C, N_FFT, HOP * GQ_MAX_FRAMES, HOWL_GRU_MAX_LABELS);
    HOWL_STREAM_REQUIRE_GEOMETRY("howl_gru_stream_windows", N, HOWL_GRU_STREAM_MAX_WINDOWS, ld, L_samples);
    const GqGeom gm = gq_geom(L_samples);
    HOWL_REQUIRE(frames >= 1 && frames <= gm.T, "howl_gru_stream_windows: frames=%d outside 1..%d (T = 1 + L / %d)", frames, gm.T, HOP);
    HOWL_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "howl_gru_stream_windows: ws must be 4-byte aligned");
    const size_t need = (size_t)N * (size_t)gm.ws_floats * sizeof(float);
    if (ws_bytes < need) {
        howl_set_error("howl_gru_stream_windows: workspace too small (%zu < %zu bytes)", ws_bytes, need);
        return HOWL_E_WORKSPACE;
    }
    const int nsteps = (frames + 4) / 2 < gm.T1 ? (frames + 4) / 2 : gm.T1;
    const int aligned = stream_pcm_aligned(pcm, ld, N);
    const GqModel model{*prm, buffers->bn1_mean, buffers->bn1_var, buffers->bn2_mean, buffers->bn2_var};
    constexpr size_t lds = (size_t)GQ_LDS_FLOATS * sizeof(float);
    static thread_local size_t granted[16] = {};
    howl_raise_lds(reinterpret_cast<const void*>(gru_stream_kernel), lds, granted, "howl_gru_stream_windows");
    hipLaunchKernelGGL(gru_stream_kernel, dim3((unsigned)N), dim3(GQ_THREADS), lds, stream, model, pcm, ld, L_samples, nsteps, fbp, log_eps,
                       zmuv_pair, aligned, C, probs, logits, static_cast<float*>(ws));
    HOWL_CHECK_LAUNCH("howl_gru_stream_windows");
    return HOWL_OK;
}

}  // extern "C"
