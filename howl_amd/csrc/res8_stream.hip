// Streaming res8 (include/howl_hip_stream.h): ONE launch from a window's raw PCM to its class probabilities, one workgroup per
// window, no activation ever leaves the compute unit.  Replaces, for the live client's window (inference.py:247-267), the chain
// howl_logmel_fwd -> howl_res8_fwd (bn_eval_stats, conv0, six conv3x3, head) -> softmax: about eleven launches for ~30 MFLOP.
//
// Per workgroup, with workgroup barriers only (nothing is shared between workgroups, so there is no counter, flag or spin loop):
//   1. log-mel + ZMUV of the window (logmel_body of howl_logmel.hip.h, standard filterbank) straight into a zero-haloed LDS tile;
//   2. conv0 (1 -> 45, 3x3) + ReLU + AvgPool(3,4) on the matrix cores -> the pooled map in LDS (conv0_fwd_mfma_kernel's tile form);
//   3. six 45 -> 45 3x3 layers as GEMMs position x cout over K = 405 (v_mfma_f32_16x16x4_f32, exact fp32): A fragments read from
//      the LDS map, B fragments (packed once by howl_res8_stream_prepare, res8.hip's wp_fwd order) from global memory / L2;
//      ReLU, the residual add of layers 2/4/6 and eval-mode BatchNorm in the epilogue (cnn.py:127-145);
//   4. spatial mean -> Linear(45, C) -> softmax.
//
// LDS plan.  ONE activation map, not three: a layer's whole output lives in its waves' accumulators (<= 6 tiles of 16 positions x
// 48 channels per wave), so after a barrier it is written back IN PLACE over its own input; the residual stream (the pre-BatchNorm
// sum that layers 2/4/6 add to) has the accumulators' lane mapping and stays in registers as well.  The map is [45 channels][PL]
// with plane pitch PL = 16 (mod 32) (the four K lane groups of a ds_read_b32 fall on disjoint banks), a plane being the pooled rows
// with a zero halo: position (r, c) at 12 (r + 1) + (c + 1), so a 3x3 tap is a constant offset and the GEMM's M dimension is simply
// the flat index q = 12 r + cc over the rows WITH their halo columns (12/10 of the arithmetic, no per-tap masks).  Halo outputs
// are computed on junk and written as zeros, which is what keeps the halo zero for the next layer.
//   windows up to 41 frames (13 pooled rows; the client's 500 ms): 8 waves, <= 2 position tiles per wave
//     static 98,048 B (logmel_body<8>: 74,752 transpose tiles + 5,888 tables + 17,408 filterbank fragments) + dynamic <= 46.5 KB
//   up to 83 frames (27 rows; 1 s): 4 waves (the frontend's transpose tiles are per wave: 37,376 B), <= 6 tiles per wave
//     static 60,672 B + dynamic <= 83 KB
#include "howl_logmel.hip.h"
#include "howl_stream.hip.h"
#include "../../include/howl_hip_stream.h"

namespace {

constexpr int SR_NMAP = 45;          // res8 feature maps (cnn.py:110)
constexpr int SR_CP = 48;            // ... padded to three MFMA tiles
constexpr int SR_MELS = 40;
constexpr int SR_PW = 10;            // pooled width = 40 mels / 4
constexpr int SR_RP = 12;            // row pitch of a plane: 10 + left / right halo
constexpr int SR_ORG = SR_RP;        // plane offset of q = 0: one halo row above
constexpr int SR_KFULL = 11;         // full blocks of four input channels (nine k-steps each: one per tap)
constexpr int SR_KSTEPS = 9 * SR_KFULL + 3;   // + channel 44 alone: its nine taps as three k-steps (res8.hip's KSTEPS)
constexpr int SR_KPAD = 9 * (SR_KFULL + 1);   // k-steps stored per cout tile: twelve whole blocks (the last six are zeros), so that
                                              // the K loop requests every block, the short one included, in one shape
constexpr int SR_MAX_ROWS = 27;
constexpr int SR_MAX_FRAMES = 83;
constexpr int SR_FP = SR_MELS + 4;   // feature tile pitch (conv0_fwd_mfma_kernel's tile: halo column each side + 2 slack)
constexpr float SR_BN_EPS = 1e-5f;
constexpr int SR_LEAD = 4, SR_TAIL = 32;      // floats in front of / behind the map that junk rows may read (finite: zeroed)

// prepared state, in floats
constexpr int SR_WP_LAYER = 3 * SR_KPAD * 64;            // wp[nt][kstep][lane]
constexpr int SR_ST_WP = 0;
constexpr int SR_ST_BN = SR_ST_WP + 6 * SR_WP_LAYER;     // [layer][mean | rstd][48]
constexpr int SR_ST_W0 = SR_ST_BN + 6 * 2 * SR_CP;       // conv0 B fragments [ks][nt][lane]
constexpr int SR_ST_OW = SR_ST_W0 + 3 * 3 * 64;          // output.weight (C, 45), then output.bias (C)
__host__ __device__ inline size_t sr_state_floats(int C) { return (size_t)SR_ST_OW + (size_t)C * (SR_NMAP + 1); }

struct SrParams {
    const float* conv0_w;
    const float* conv_w[6];
    const float* mean[6];
    const float* var[6];
    const float* out_w;
    const float* out_b;
};

__global__ __launch_bounds__(256) void res8_stream_prepare_kernel(SrParams p, int C, float* __restrict__ st) {
    const int total = (int)sr_state_floats(C);
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        float v = 0.0f;
        if (e < SR_ST_BN) {
            // B[k][n] = w[cout = 16 nt + n][cin][tap]: block c0 of four channels with one tap per k-step, then channel 44 whose k
            // walks four taps per k-step (taps 9..11 are padding)
            const int layer = e / SR_WP_LAYER, idx = e - layer * SR_WP_LAYER;
            const int lane = idx & 63, ks = (idx >> 6) % SR_KPAD, nt = idx / (64 * SR_KPAD);
            int kk, tap;
            if (ks < 9 * SR_KFULL) {
                const int c0 = ks / 9;
                tap = ks - 9 * c0;
                kk = 4 * c0 + (lane >> 4);
            } else {
                tap = 4 * (ks - 9 * SR_KFULL) + (lane >> 4);
                kk = 4 * SR_KFULL;
            }
            const int n = 16 * nt + (lane & 15);
            if (ks < SR_KSTEPS && kk < SR_NMAP && n < SR_NMAP && tap < 9) v = p.conv_w[layer][(n * SR_NMAP + kk) * 9 + tap];
        } else if (e < SR_ST_W0) {
            const int i = e - SR_ST_BN, layer = i / (2 * SR_CP), c = i % SR_CP;
            const bool rstd = (i / SR_CP) & 1;
            if (c < SR_NMAP) v = rstd ? 1.0f / sqrtf(p.var[layer][c] + SR_BN_EPS) : p.mean[layer][c];
        } else if (e < SR_ST_OW) {
            const int i = e - SR_ST_W0, lane = i & 63, nt = (i >> 6) % 3, ks = i / (3 * 64);
            const int tap = 4 * ks + (lane >> 4), c = 16 * nt + (lane & 15);
            if (tap < 9 && c < SR_NMAP) v = p.conv0_w[c * 9 + tap];
        } else {
            const int i = e - SR_ST_OW;
            v = i < C * SR_NMAP ? p.out_w[i] : p.out_b[i - C * SR_NMAP];
        }
        st[e] = v;
    }
}

// plane offset of tap (kh, kw) relative to the output position
__host__ __device__ constexpr int sr_tap_off(int tap) { return (tap / 3 - 1) * SR_RP + (tap % 3 - 1); }

// The K loop of one layer for the NUV position tiles of this wave: per k-step three B fragments (one per cout tile) from global
// memory and one A fragment per position tile from the LDS map, 3 NUV MFMAs.  The B fragments of a block of four input channels
// (nine k-steps) are requested one block ahead: their latency is spent under the 27 NUV MFMAs of the block in hand instead of in
// front of every block -- with the loads inside the block the loop was a chain of 72 exposed L2 round trips per window (the
// launch took 194 us that way and 162 with the requests a block ahead).
template <int NU, int NUV>
__device__ __forceinline__ void sr_kloop(f32x4 (&acc)[NU][3], const float* __restrict__ wl, const float* amap, int PL,
                                         const int (&q0)[NU], int lane) {
    const int g = lane >> 4, n = lane & 15;
    const float* ap = amap + g * PL + SR_ORG + n;
    const float* wk = wl + lane;
    float bn[9][3];      // the next block's fragments
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int nt = 0; nt < 3; ++nt) bn[tap][nt] = wk[(nt * SR_KPAD + tap) * 64];
#pragma unroll 1
    for (int c0 = 0; c0 < SR_KFULL; ++c0) {
        float b[9][3];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int nt = 0; nt < 3; ++nt) b[tap][nt] = bn[tap][nt];
        __builtin_amdgcn_sched_barrier(0);      // (and the hand-over stays here, a whole block behind its requests)
        wk += 9 * 64;      // (behind the last full block: channel 44's three k-steps and six of padding)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int nt = 0; nt < 3; ++nt) bn[tap][nt] = wk[(nt * SR_KPAD + tap) * 64];
        __builtin_amdgcn_sched_barrier(0);      // the requests stay up here: sunk between the MFMAs they were waited for at once
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
            for (int j = 0; j < NUV; ++j) {
                const float a = ap[q0[j] + sr_tap_off(tap)];
#pragma unroll
                for (int nt = 0; nt < 3; ++nt) acc[j][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[tap][nt], acc[j][nt], 0, 0, 0);
            }
        }
        ap += 4 * PL;
    }
    // channel 44: k = g walks taps 4 s + g; taps 9..11 meet zero weights, any FINITE value will do: tap 8's
    const float* at = amap + (SR_NMAP - 1) * PL + SR_ORG + n;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int tap = min(4 * s + g, 8);
        const int off = (tap / 3 - 1) * SR_RP + (tap % 3 - 1);
#pragma unroll
        for (int j = 0; j < NUV; ++j) {
            const float a = at[q0[j] + off];
#pragma unroll
            for (int nt = 0; nt < 3; ++nt) acc[j][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bn[s][nt], acc[j][nt], 0, 0, 0);
        }
    }
}
template <int NU, int NUV = NU>
__device__ __forceinline__ void sr_kloop_n(int nu, f32x4 (&acc)[NU][3], const float* __restrict__ wl, const float* amap, int PL,
                                           const int (&q0)[NU], int lane) {
    if constexpr (NUV >= 1) {
        if (nu == NUV)      // (wave-uniform)
            sr_kloop<NU, NUV>(acc, wl, amap, PL, q0, lane);
        else
            sr_kloop_n<NU, NUV - 1>(nu, acc, wl, amap, PL, q0, lane);
    }
}

// NW waves; NU = position tiles (16 flat positions x 48 channels) a wave may hold: tile mt belongs to wave mt % NW.
template <int NW, int NU>
__global__ __launch_bounds__(NW * 64) void res8_stream_kernel(const float* __restrict__ state, const float* __restrict__ pcm, long ld,
                                                            int L, int T, int R, int PL, int feat_floats,
                                                            const float* __restrict__ fbp, float log_eps,
                                                            const float* __restrict__ zmuv, int aligned, int C,
                                                            float* __restrict__ probs, float* __restrict__ logits) {
    HIP_DYNAMIC_SHARED(float, lds)
    float* const feat = lds;                                   // (T + 2) x 44 feature tile, zero halo, + slack
    float* const amap = lds + feat_floats + SR_LEAD;           // [45][PL]
    float* const pooled = amap + SR_NMAP * PL + SR_TAIL;       // [48]
    float* const lg = pooled + SR_CP;                          // [64]
    const int total_floats = feat_floats + SR_LEAD + SR_NMAP * PL + SR_TAIL + SR_CP + HOWL_STREAM_MAX_CLASSES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, n = lane & 15;
    const long win = blockIdx.x;

    // everything the later stages read without having written it (halos, slack, junk rows' neighbourhood) is zero
    for (int i = tid; i < total_floats / 4; i += NW * 64) reinterpret_cast<float4*>(lds)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

    // ---- 1. log-mel + ZMUV: frame t, mel m -> feat[(t + 1) * 44 + (m + 1)] (layout 1 with the tile pitch as the row length); the
    // body's own barrier, which precedes its first store, orders the zero fill above before them
    logmel_body<NW, NG_BANDED>(pcm + win * ld, L, ld, T, T, fbp, SR_MELS, log_eps, zmuv, feat + SR_FP + 1, 1, (T + QUAD - 1) / QUAD,
                               aligned, 0u, 1u, SR_FP);
    __syncthreads();

    // ---- 2. conv0 + ReLU + AvgPool(3,4).  A 16-row tile is 8 mel bins (two pooled cells) of one frame of TWO consecutive pooled
    // rows; the three frames of a cell are three tiles accumulated by the same lanes, and a lane holds the 4 mel bins of one cell
    // (rows 4 g + r): ReLU and the 3 x 4 sum are lane-local (conv0_fwd_mfma_kernel).
    {
        float bw[3][3];
        int aoff[3];
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
#pragma unroll
            for (int nt = 0; nt < 3; ++nt) bw[ks][nt] = state[SR_ST_W0 + (ks * 3 + nt) * 64 + lane];
            const int tap = min(4 * ks + g, 8);      // taps 9..11 meet zero weights
            aoff[ks] = (tap / 3) * SR_FP + tap % 3 + (n & 7) + (n >> 3) * 3 * SR_FP;
        }
        for (int u = wave; u < 5 * ((R + 1) / 2); u += NW) {
            const int pp = u / 5, j8 = u - 5 * pp;
            const float* rowp = feat + 3 * (2 * pp) * SR_FP + 8 * j8;
            f32x4 acc[3][3];      // [frame tl][cout tile nt]
#pragma unroll
            for (int tl = 0; tl < 3; ++tl)
#pragma unroll
                for (int nt = 0; nt < 3; ++nt) acc[tl][nt] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int tl = 0; tl < 3; ++tl)
#pragma unroll
                for (int ks = 0; ks < 3; ++ks) {
                    const float a = rowp[aoff[ks] + tl * SR_FP];
#pragma unroll
                    for (int nt = 0; nt < 3; ++nt) acc[tl][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bw[ks][nt], acc[tl][nt], 0, 0, 0);
                }
            const int pw = 2 * j8 + (g & 1), ph = 2 * pp + (g >> 1);      // this lane's cell
#pragma unroll
            for (int nt = 0; nt < 3; ++nt) {
                float sum = 0.0f;
#pragma unroll
                for (int tl = 0; tl < 3; ++tl)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sum += fmaxf(acc[tl][nt][r], 0.0f);
                const int c = 16 * nt + n;
                if (ph < R && c < SR_NMAP) amap[c * PL + SR_ORG + ph * SR_RP + pw + 1] = sum * (1.0f / 12.0f);
            }
        }
    }
    __syncthreads();

    // ---- 3. the six 3x3 layers.  This wave's position tiles and, per tile and cout tile, four outputs per lane: flat positions
    // q = 16 mt + 4 g + r (one pooled row: 12 is a multiple of 4) of channel 16 nt + n.
    const int MT = (R * SR_RP + 15) / 16;
    int q0[NU];
    int nu = 0;
#pragma unroll
    for (int j = 0; j < NU; ++j) {
        const int mt = wave + NW * j;
        q0[j] = 16 * (mt < MT ? mt : 0);
        nu += mt < MT ? 1 : 0;
    }
    f32x4 res[NU][3];      // the residual stream (cnn.py's old_x): conv0's pooled output first
#pragma unroll
    for (int j = 0; j < NU; ++j)
#pragma unroll
        for (int nt = 0; nt < 3; ++nt) {
            const int c = 16 * nt + n;
            res[j][nt] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (j < nu && c < SR_NMAP) res[j][nt] = *reinterpret_cast<const f32x4*>(amap + c * PL + SR_ORG + q0[j] + 4 * g);
        }
#pragma unroll 1
    for (int layer = 0; layer < 6; ++layer) {
        f32x4 acc[NU][3];
#pragma unroll
        for (int j = 0; j < NU; ++j)
#pragma unroll
            for (int nt = 0; nt < 3; ++nt) acc[j][nt] = {0.0f, 0.0f, 0.0f, 0.0f};
        sr_kloop_n<NU>(nu, acc, state + SR_ST_WP + layer * SR_WP_LAYER, amap, PL, q0, lane);
        const bool add = (layer & 1) != 0;      // layers 2, 4, 6 (counted from 1)
        const bool last = layer == 5;           // its BatchNorm is applied to the spatial mean (affine-free: the same thing)
        float mean[3], rstd[3];
#pragma unroll
        for (int nt = 0; nt < 3; ++nt) {
            mean[nt] = state[SR_ST_BN + (layer * 2 + 0) * SR_CP + 16 * nt + n];
            rstd[nt] = state[SR_ST_BN + (layer * 2 + 1) * SR_CP + 16 * nt + n];
        }
        __syncthreads();      // every wave has read its A fragments: the map may be overwritten
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            if (j >= nu) continue;      // (wave-uniform)
            const int qb = q0[j] + 4 * g, rr = qb / SR_RP, cc0 = qb - rr * SR_RP;
#pragma unroll
            for (int nt = 0; nt < 3; ++nt) {
                f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float y = fmaxf(acc[j][nt][r], 0.0f);
                    if (add) {
                        y += res[j][nt][r];
                        res[j][nt][r] = y;
                    }
                    const bool inside = rr < R && cc0 + r >= 1 && cc0 + r <= SR_PW;
                    const float v = last ? y : (y - mean[nt]) * rstd[nt];
                    o[r] = inside ? v : 0.0f;      // halo and tail positions stay zero for the next layer
                }
                if (16 * nt + n < SR_NMAP) *reinterpret_cast<f32x4*>(amap + (16 * nt + n) * PL + SR_ORG + qb) = o;
            }
        }
        __syncthreads();
    }

    // ---- 4. spatial mean (of the pre-BatchNorm map, then BatchNorm 6) -> Linear -> softmax
    // eight threads per channel (lanes 8 k .. 8 k + 7 of a wave), folded by three shuffles; NW * 8 channels per trip
    const int P = R * SR_PW;
    for (int c0 = 0; c0 < SR_NMAP; c0 += NW * 8) {
        const int c = c0 + (tid >> 3), part = tid & 7;
        const bool real = c < SR_NMAP;
        const float bm = real ? state[SR_ST_BN + (5 * 2 + 0) * SR_CP + c] : 0.0f;
        const float br = real ? state[SR_ST_BN + (5 * 2 + 1) * SR_CP + c] : 0.0f;
        double s = 0.0;
        if (real)
            for (int i = part; i < P; i += 8) {
                const int r = i / SR_PW, cc = i - r * SR_PW;
                s += (double)amap[c * PL + SR_ORG + r * SR_RP + cc + 1];
            }
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        if (real && part == 0) pooled[c] = ((float)(s / (double)P) - bm) * br;
    }
    __syncthreads();
    if (tid < C) {
        const float* ow = state + SR_ST_OW + tid * SR_NMAP;
        float a = state[SR_ST_OW + C * SR_NMAP + tid];
        for (int c = 0; c < SR_NMAP; ++c) a = fmaf(ow[c], pooled[c], a);
        lg[tid] = a;
        if (logits != nullptr) logits[win * C + tid] = a;
    }
    __syncthreads();
    if (tid < C) {
        float mx = lg[0];
        for (int k = 1; k < C; ++k) mx = fmaxf(mx, lg[k]);
        float se = 0.0f;
        for (int k = 0; k < C; ++k) se += expf(lg[k] - mx);
        probs[win * C + tid] = expf(lg[tid] - mx) / se;
    }
}

struct SrPlan {
    int T, R, PL, feat_floats;
    size_t lds;
    bool small;      // the eight-wave instance
};
SrPlan sr_plan(int L) {
    SrPlan p;
    p.T = 1 + L / HOP;
    p.R = p.T / 3;
    const int MT = (p.R * SR_RP + 15) / 16;
    // a plane holds the rows with their halo and every tile's outputs; pitch = 16 (mod 32)
    const int rows = (p.R + 2) * SR_RP, tiles = SR_ORG + 16 * MT;
    const int need = rows > tiles ? rows : tiles;
    p.PL = ((need + 15) / 32) * 32 + 16;
    p.feat_floats = ((p.T + 2) * SR_FP + 3 * SR_FP + 16 + 3) & ~3;      // + the rows an odd last row pair reads (conv0_tile_floats)
    p.lds = (size_t)(p.feat_floats + SR_LEAD + SR_NMAP * p.PL + SR_TAIL + SR_CP + HOWL_STREAM_MAX_CLASSES) * sizeof(float);
    p.small = MT <= 2 * 8 && p.R <= 13;
    return p;
}
bool sr_supported(int L, int M, int C) {
    return M == SR_MELS && C >= 1 && C <= HOWL_STREAM_MAX_CLASSES && L > N_FFT / 2 && 1 + L / HOP >= 3 && 1 + L / HOP <= SR_MAX_FRAMES;
}

template <int NW, int NU>
void sr_launch(const SrPlan& p, int N, hipStream_t stream, const float* state, const float* pcm, long ld, int L, const float* fbp,
               float log_eps, const float* zmuv, int aligned, int C, float* probs, float* logits) {
    static thread_local size_t granted[16] = {};
    howl_raise_lds(reinterpret_cast<const void*>(res8_stream_kernel<NW, NU>), p.lds, granted, "howl_res8_stream_windows");
    hipLaunchKernelGGL((res8_stream_kernel<NW, NU>), dim3((unsigned)N), dim3(NW * 64), p.lds, stream, state, pcm, ld, L, p.T, p.R, p.PL,
                       p.feat_floats, fbp, log_eps, zmuv, aligned, C, probs, logits);
}

}  // namespace

extern "C" {

int howl_res8_stream_supported(int L_samples, int M, int C) { return sr_supported(L_samples, M, C) ? 1 : 0; }

size_t howl_res8_stream_state_bytes(int C) {
    return C >= 1 && C <= HOWL_STREAM_MAX_CLASSES ? sr_state_floats(C) * sizeof(float) : 0;
}

int howl_res8_stream_prepare(const HowlRes8Params* prm, int C, void* state, size_t state_bytes, hipStream_t stream) {
    HOWL_REQUIRE(prm && state, "howl_res8_stream_prepare: null pointer");
    HOWL_REQUIRE(C >= 1 && C <= HOWL_STREAM_MAX_CLASSES, "howl_res8_stream_prepare: C=%d unsupported (1..%d)", C, HOWL_STREAM_MAX_CLASSES);
    HOWL_REQUIRE(state_bytes >= sr_state_floats(C) * sizeof(float), "howl_res8_stream_prepare: state of %zu bytes, C=%d needs %zu",
                 state_bytes, C, sr_state_floats(C) * sizeof(float));
    SrParams p;
    p.conv0_w = prm->conv0_w;
    p.out_w = prm->out_w;
    p.out_b = prm->out_b;
    bool all = p.conv0_w && p.out_w && p.out_b;
    for (int i = 0; i < 6; ++i) {
        p.conv_w[i] = prm->conv_w[i];
        p.mean[i] = prm->bn_running_mean[i];
        p.var[i] = prm->bn_running_var[i];
        all = all && p.conv_w[i] && p.mean[i] && p.var[i];
    }
    HOWL_REQUIRE(all, "howl_res8_stream_prepare: null pointer in HowlRes8Params");
    const int total = (int)sr_state_floats(C);
    hipLaunchKernelGGL(res8_stream_prepare_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, p, C, static_cast<float*>(state));
    HOWL_CHECK_LAUNCH("howl_res8_stream_prepare");
    return HOWL_OK;
}

int howl_res8_stream_windows(const void* state, const float* pcm, long ld, int N, int L_samples, const float* fbp, int M,
                             float log_eps, const float* zmuv_pair, int C, float* probs, float* logits, hipStream_t stream) {
    HOWL_REQUIRE(state && pcm && fbp && probs, "howl_res8_stream_windows: null pointer");
    HOWL_REQUIRE(sr_supported(L_samples, M, C),
                 "howl_res8_stream_windows: L=%d samples, M=%d, C=%d unsupported (M = 40, 3..%d frames, C <= %d: howl_res8_stream_supported)",
                 L_samples, M, C, SR_MAX_FRAMES, HOWL_STREAM_MAX_CLASSES);
    HOWL_STREAM_REQUIRE_GEOMETRY("howl_res8_stream_windows", N, HOWL_STREAM_MAX_WINDOWS, ld, L_samples);
    const SrPlan p = sr_plan(L_samples);
    const int aligned = stream_pcm_aligned(pcm, ld, N);
    if (p.small)
        sr_launch<8, 2>(p, N, stream, static_cast<const float*>(state), pcm, ld, L_samples, fbp, log_eps, zmuv_pair, aligned, C, probs, logits);
    else
        sr_launch<4, 6>(p, N, stream, static_cast<const float*>(state), pcm, ld, L_samples, fbp, log_eps, zmuv_pair, aligned, C, probs, logits);
    HOWL_CHECK_LAUNCH("howl_res8_stream_windows");
    return HOWL_OK;
}

}  // extern "C"
