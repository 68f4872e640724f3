// Streaming las (include/howl_hip_las_stream.h): ONE launch from a window's raw PCM to its class probabilities, one workgroup of
// twelve waves per window.  Replaces, for the live client's window (inference.py:247-267), the chain howl_logmel_fwd ->
// howl_deltas_fwd -> howl_las_fwd (conv1, conv2, features, two GEMMs, the recurrence, two GEMMs, attention, head) -> softmax:
// thirteen launches for about 10 MFLOP.  The model is the eval-mode model of las.hip with its order of operations.
//
// Per workgroup, with workgroup barriers only (nothing is shared between workgroups, so there is no counter, flag or spin loop):
//   1. log-mel of the window's T frames (logmel_body<8> of howl_logmel.hip.h on waves 0..7, standard filterbank, no ZMUV) into LDS;
//   2. deltas and accelerations (deltas_kernel's arithmetic) + ZMUV -> three zero-bordered feature planes in LDS;
//   3. conv1 + BN1 + ReLU + MaxPool(1,2), one pooled position and eight channels per thread -> the pooled map with its zero
//      border in the window's workspace;
//   4. conv2 + BN2 + ReLU + pool, one step's row and eight channels per thread -> the features F (T2, 352) in LDS;
//   5. Gx = F W_ih^T + b_ih + b_hh of both directions on v_mfma_f32_16x16x4_f32 (exact fp32): A fragments from F, B fragments
//      from the prepared state, requested a block of eight k-steps ahead of their MFMAs -> the workspace;
//   6. both directions side by side, n dependent steps: waves 0..5 forward, 6..11 reverse (from zero state at step n - 1); thread =
//      one gate row with its 96 W_hh values in registers, h through LDS, the four gates of a unit meet inside a quad of lanes
//      (DPP), one barrier per step, Gx three steps ahead;
//   7. V and K projections on the matrix cores -> LDS;  8. attention, one wave per head, one pass with a running maximum;
//   9. Linear(192,256) - ReLU - Linear(256,C);  10. softmax.
//
// LDS plan (floats; the regions of a later phase lie over the dead ones of an earlier one).  Static: logmel_body<8> 98,048 B.
//   phases 1-3: log-mels [T][40] 3,320 | features [3][44][PW] 11,484 (PW = T + 4, odd) | conv weights and folded BatchNorms 840
//   phases 4-5: F [32][354] 11,328 (rows >= T2 are junk that only junk output rows see) | conv weights
//   phases 6-10: h sequence [32][194] 6,208 | h double buffer 384 | V,K [22][388] 8,536 | ctx 192 | y1 256 | logits 64
// = 15,644 floats = 62,576 B dynamic, 160,624 of 163,840 B in all.  The pooled conv1 map (<= 67.7 KB with its border) and Gx
// (<= 67.6 KB) do not fit beside that: they go through `ws`, each window's share written and read back by its own workgroup only,
// between workgroup barriers.
#include "howl_logmel.hip.h"
#include "howl_lstm.hip.h"
#include "howl_stream.hip.h"
#include "../../include/howl_hip_las_stream.h"

namespace {

constexpr int LQ_H = 96, LQ_G = 4 * LQ_H, LQ_D = 2 * LQ_H;
constexpr int LQ_M = 40, LQ_R1 = LQ_M + 2, LQ_R2 = LQ_M + 4, LQ_RP = LQ_R1 + 4;      // rows of conv1's / conv2's output, of the bordered map
constexpr int LQ_F = 8 * LQ_R2;              // 352 LSTM input features, index channel * 44 + mel
constexpr int LQ_HD = 256, LQ_HEADS = 4, LQ_HW = LQ_D / LQ_HEADS;
constexpr int LQ_THREADS = 768, LQ_WAVES = 12, LQ_FE_WAVES = 8;
constexpr int LQ_MAX_FRAMES = 83;
constexpr int LQ_KS_IH = LQ_F / 4, LQ_KS_VK = LQ_D / 4, LQ_KB = 8;      // k-steps of the two GEMMs, k-steps per requested block
constexpr float LQ_BN_EPS = 1e-5f;
static_assert(LQ_KS_IH % LQ_KB == 0 && LQ_KS_VK % LQ_KB == 0, "whole blocks of k-steps");

// prepared state, in floats
constexpr int LQ_ST_C1W = 0;                           // [(ch * 9 + tap) * 8 + co]
constexpr int LQ_ST_C1A = LQ_ST_C1W + 216;             // bias[8] | scale[8] | shift[8]
constexpr int LQ_ST_C2W = LQ_ST_C1A + 24;              // [(ci * 9 + tap) * 8 + co]
constexpr int LQ_ST_C2A = LQ_ST_C2W + 576;
constexpr int LQ_ST_CONV = LQ_ST_C2A + 24;             // (the 840 floats above are copied to LDS as one piece)
constexpr int LQ_ST_CV = LQ_ST_CONV;                   // context_vec[192]
constexpr int LQ_ST_BG = LQ_ST_CV + LQ_D;              // b_ih + b_hh [dir][384]
constexpr int LQ_ST_VKB = LQ_ST_BG + 2 * LQ_G;         // v_b | k_b
constexpr int LQ_ST_B1 = LQ_ST_VKB + 2 * LQ_D;
constexpr int LQ_ST_WHH = LQ_ST_B1 + LQ_HD;            // [dir][k / 4][thread of 384][4]
constexpr int LQ_ST_WIH = LQ_ST_WHH + 2 * LQ_G * LQ_H;               // B fragments [48 column tiles][88 k-steps][lane]
constexpr int LQ_ST_VK = LQ_ST_WIH + 48 * LQ_KS_IH * 64;             // B fragments [24][48][lane]: V's columns, then K's
constexpr int LQ_ST_W1T = LQ_ST_VK + 24 * LQ_KS_VK * 64;             // fc.0.weight transposed [192][256]
constexpr int LQ_ST_W2 = LQ_ST_W1T + LQ_D * LQ_HD;                   // fc.3.weight (C, 256), then fc.3.bias (C)
static_assert(LQ_ST_WHH % 4 == 0, "16-byte loads of the recurrence's weights");
__host__ __device__ inline size_t lq_state_floats(int C) { return (size_t)LQ_ST_W2 + (size_t)C * (LQ_HD + 1); }

// dynamic LDS, in floats
constexpr int LQ_FP = LQ_F + 2;              // F's row pitch = 2 (mod 32): the A fragment's 16 rows x 2 k of a lane half on 32 banks
constexpr int LQ_HP = LQ_D + 2;              // the h sequence's, likewise
constexpr int LQ_VP = 2 * LQ_D + 4;
constexpr int LQ_L_LM = 0;
constexpr int LQ_L_X3 = LQ_L_LM + LQ_MAX_FRAMES * LQ_M;
constexpr int LQ_L_CW = LQ_L_X3 + 3 * LQ_R2 * (LQ_MAX_FRAMES + 4);
constexpr int LQ_L_F = 0;
constexpr int LQ_L_HS = 0;
constexpr int LQ_L_HB = LQ_L_HS + 32 * LQ_HP;
constexpr int LQ_L_VK = LQ_L_HB + 2 * LQ_D;
constexpr int LQ_L_CTX = LQ_L_VK + 22 * LQ_VP;
constexpr int LQ_L_Y1 = LQ_L_CTX + LQ_D;
constexpr int LQ_L_LG = LQ_L_Y1 + LQ_HD;
constexpr int LQ_LDS_FLOATS = LQ_L_CW + LQ_ST_CONV;
static_assert(32 * LQ_FP <= LQ_L_CW, "F (with its junk rows) ends in front of the conv weights");
static_assert(LQ_L_LG + HOWL_LAS_MAX_LABELS <= LQ_LDS_FLOATS, "the last phases fit the allocation");

struct LqGeom {
    int T, W1, T1, W2, T2;
    int p1_floats, ws_floats;      // the bordered pooled map [8][T1 + 4][46]; the window's whole share (+ Gx [T2][768])
};
__host__ __device__ inline LqGeom lq_geom(int L) {
    LqGeom g;
    g.T = 1 + L / HOP;
    g.W1 = g.T + 2;
    g.T1 = g.W1 / 2;
    g.W2 = g.T1 + 2;
    g.T2 = g.W2 / 2;
    g.p1_floats = 8 * (g.T1 + 4) * LQ_RP;
    g.ws_floats = (g.p1_floats + g.T2 * 2 * LQ_G + 3) & ~3;
    return g;
}

struct LqPrep {
    HowlLasParams p;
    const float *m1, *v1, *m2, *v2;
};

__global__ __launch_bounds__(256) void las_stream_prepare_kernel(LqPrep a, int C, float* __restrict__ st) {
    const HowlLasParams& p = a.p;
    const int total = (int)lq_state_floats(C);
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        float v;
        if (e < LQ_ST_C1A) {
            v = p.conv1_w[(e & 7) * 27 + (e >> 3)];
        } else if (e < LQ_ST_C2W || (e >= LQ_ST_C2A && e < LQ_ST_CONV)) {
            const bool two = e >= LQ_ST_C2A;
            const int i = e - (two ? LQ_ST_C2A : LQ_ST_C1A), c = i & 7;
            // y = z * sc + sh (las.hip's bn_affine from the running statistics)
            const float sc = (two ? p.bn2_w : p.bn1_w)[c] * (1.0f / sqrtf((two ? a.v2 : a.v1)[c] + LQ_BN_EPS));
            v = i < 8 ? (two ? p.conv2_b : p.conv1_b)[c] : (i < 16 ? sc : (two ? p.bn2_b : p.bn1_b)[c] - (two ? a.m2 : a.m1)[c] * sc);
        } else if (e < LQ_ST_C2A) {
            const int i = e - LQ_ST_C2W;
            v = p.conv2_w[(i & 7) * 72 + (i >> 3)];
        } else if (e < LQ_ST_BG) {
            v = p.cv[e - LQ_ST_CV];
        } else if (e < LQ_ST_VKB) {
            const int i = e - LQ_ST_BG, r = i % LQ_G;
            v = i < LQ_G ? p.b_ih_f[r] + p.b_hh_f[r] : p.b_ih_r[r] + p.b_hh_r[r];
        } else if (e < LQ_ST_B1) {
            const int i = e - LQ_ST_VKB;
            v = i < LQ_D ? p.v_b[i] : p.k_b[i - LQ_D];
        } else if (e < LQ_ST_WHH) {
            v = p.b1[e - LQ_ST_B1];
        } else if (e < LQ_ST_WIH) {
            // thread t of a direction's 384: wave c = t / 64, lane 4 j + g = gate g of unit 16 c + j
            const int i = e - LQ_ST_WHH, k = i & 3, t = (i >> 2) % LQ_G, q = ((i >> 2) / LQ_G) % (LQ_H / 4), dir = i / (LQ_G * LQ_H);
            const int row = (t & 3) * LQ_H + 16 * (t >> 6) + ((t & 63) >> 2);
            v = (dir ? p.w_hh_r : p.w_hh_f)[row * LQ_H + 4 * q + k];
        } else if (e < LQ_ST_VK) {
            // B[k][n] = W_ih[n][k] over the 768 gate rows of both directions
            const int i = e - LQ_ST_WIH, lane = i & 63, ks = (i >> 6) % LQ_KS_IH, nt = i / (64 * LQ_KS_IH);
            const int k = 4 * ks + (lane >> 4), col = 16 * nt + (lane & 15);
            v = (col < LQ_G ? p.w_ih_f : p.w_ih_r)[(col % LQ_G) * LQ_F + k];
        } else if (e < LQ_ST_W1T) {
            const int i = e - LQ_ST_VK, lane = i & 63, ks = (i >> 6) % LQ_KS_VK, nt = i / (64 * LQ_KS_VK);
            const int k = 4 * ks + (lane >> 4), col = 16 * nt + (lane & 15);
            v = (col < LQ_D ? p.v_w : p.k_w)[(col % LQ_D) * LQ_D + k];
        } else if (e < LQ_ST_W2) {
            const int i = e - LQ_ST_W1T;
            v = p.w1[(i % LQ_HD) * LQ_D + i / LQ_HD];
        } else {
            const int i = e - LQ_ST_W2;
            v = i < C * LQ_HD ? p.w2[i] : p.b2[i - C * LQ_HD];
        }
        st[e] = v;
    }
}

// acc[mt][j] += A[16 mt + row][k] B[k][column tile j] over KS k-steps of four, this wave's NT column tiles.  a0 = the lane's A
// address of k-step 0 (row lane & 15, k lane >> 4), wf = the lane's B address of (tile 0, k-step 0).  The B fragments of a block
// of LQ_KB k-steps are requested one block ahead: their latency is spent under the MFMAs of the block in hand instead of in front
// of every k-step (res8_stream.hip's sr_kloop).
template <int NT, int MT>
__device__ __forceinline__ void lq_gemm(f32x4 (&acc)[2][NT], const float* __restrict__ wf, int KS, const float* a0, int pitch) {
    const float* a1 = a0 + 16 * pitch;
    const int nblk = KS / LQ_KB;
    float bn[LQ_KB][NT];
#pragma unroll
    for (int ks = 0; ks < LQ_KB; ++ks)
#pragma unroll
        for (int j = 0; j < NT; ++j) bn[ks][j] = wf[(j * KS + ks) * 64];
#pragma unroll 1
    for (int blk = 0; blk < nblk; ++blk) {
        float b[LQ_KB][NT];
#pragma unroll
        for (int ks = 0; ks < LQ_KB; ++ks)
#pragma unroll
            for (int j = 0; j < NT; ++j) b[ks][j] = bn[ks][j];
        __builtin_amdgcn_sched_barrier(0);
        const int nb = min(blk + 1, nblk - 1) * LQ_KB;      // (the last block requests itself again: one shape for every trip)
#pragma unroll
        for (int ks = 0; ks < LQ_KB; ++ks)
#pragma unroll
            for (int j = 0; j < NT; ++j) bn[ks][j] = wf[(j * KS + nb + ks) * 64];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < LQ_KB; ++ks) {
            const float x0 = a0[4 * (blk * LQ_KB + ks)];
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, b[ks][j], acc[0][j], 0, 0, 0);
            if constexpr (MT == 2) {
                const float x1 = a1[4 * (blk * LQ_KB + ks)];
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, b[ks][j], acc[1][j], 0, 0, 0);
            }
        }
    }
}

// lane k of every quad of lanes -> all four
template <int K>
__device__ __forceinline__ float lq_quad_bcast(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), K * 0x55, 0xf, 0xf, true));
}

__global__ __launch_bounds__(LQ_THREADS) void las_stream_kernel(const float* __restrict__ state, const float* __restrict__ pcm, long ld,
                                                                int L, int nsteps, const float* __restrict__ fbp, float log_eps,
                                                                const float* __restrict__ zmuv, int aligned, int C,
                                                                float* __restrict__ probs, float* __restrict__ logits,
                                                                float* __restrict__ ws) {
    HIP_DYNAMIC_SHARED(float, lds)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long win = blockIdx.x;
    const LqGeom gm = lq_geom(L);
    const int T = gm.T, T1 = gm.T1, T2 = gm.T2, n = nsteps;
    const int PW = (T + 4) | 1;      // the feature planes' row pitch, odd: rows run fastest over the lanes
    float* const p1 = ws + win * gm.ws_floats;      // [ci][column + 2][row + 2], zero border (conv2's padding of 2)
    float* const gx = p1 + gm.p1_floats;            // [step][dir * 384 + gate row]
    float* const lm = lds + LQ_L_LM;
    float* const x3 = lds + LQ_L_X3;
    float* const cw = lds + LQ_L_CW;

    // what later phases read without having written it: the planes' and the map's borders
    for (int i = tid; i < 3 * LQ_R2 * PW; i += LQ_THREADS) x3[i] = 0.0f;
    for (int i = tid; i < gm.p1_floats; i += LQ_THREADS) p1[i] = 0.0f;
    for (int i = tid; i < LQ_ST_CONV; i += LQ_THREADS) cw[i] = state[i];

    // ---- 1. log-mels of the T frames: frame t, mel m -> lm[40 t + m].  The body is written for its own eight waves (one transpose
    // tile per wave) and has one workgroup barrier, which the other four waves meet here.
    if (wave < LQ_FE_WAVES)
        logmel_body<LQ_FE_WAVES, NG_BANDED>(pcm + win * ld, L, ld, T, T, fbp, LQ_M, log_eps, nullptr, lm, 1, (T + QUAD - 1) / QUAD, aligned,
                                            0u, 1u, LQ_M);
    else
        __syncthreads();
    __syncthreads();

    // ---- 2. deltas and accelerations (ComputeDeltas twice, replicate padding; deltas_kernel's arithmetic) and ZMUV
    {
        float mean = 0.0f, sd = 1.0f;
        if (zmuv != nullptr) {
            mean = zmuv[0];
            sd = zmuv[1];
        }
        for (int i = tid; i < LQ_M * T; i += LQ_THREADS) {
            const int t = i / LQ_M, m = i - t * LQ_M;
            auto clampt = [T](int u) { return u < 0 ? 0 : (u >= T ? T - 1 : u); };
            auto delta_at = [&](int u) {
                const float a = lm[clampt(u - 2) * LQ_M + m], b = lm[clampt(u - 1) * LQ_M + m], c = lm[clampt(u + 1) * LQ_M + m],
                            d = lm[clampt(u + 2) * LQ_M + m];
                return (-2.0f * a + -1.0f * b + c + 2.0f * d) / 10.0f;
            };
            const float l = lm[t * LQ_M + m];
            const float d0 = delta_at(t);
            const float dm2 = delta_at(clampt(t - 2)), dm1 = delta_at(clampt(t - 1));
            const float dp1 = delta_at(clampt(t + 1)), dp2 = delta_at(clampt(t + 2));
            const float dd = (-2.0f * dm2 + -1.0f * dm1 + dp1 + 2.0f * dp2) / 10.0f;
            float* o = x3 + (m + 2) * PW + t + 2;
            o[0] = (l - mean) / sd;
            o[LQ_R2 * PW] = (d0 - mean) / sd;
            o[2 * LQ_R2 * PW] = (dd - mean) / sd;
        }
    }
    __syncthreads();

    // ---- 3. conv1 + BN1 + ReLU + MaxPool(1,2): thread = (row h, pooled column p), the column pair x eight channels
    {
#pragma unroll 1
        for (int i = tid; i < LQ_R1 * T1; i += LQ_THREADS) {
            const int p = i / LQ_R1, h = i - p * LQ_R1;
            int wo = LQ_ST_C1W;      // opaque per item: the weights and the folded BatchNorm stay LDS broadcast reads and are not hoisted into registers of their own
            HOWL_OPAQUE_V(wo);
            const float* ca = cw + wo + (LQ_ST_C1A - LQ_ST_C1W);
            float z0[8], z1[8];
#pragma unroll
            for (int co = 0; co < 8; ++co) z0[co] = z1[co] = ca[co];
#pragma unroll 1
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const float* xr = x3 + (ch * LQ_R2 + h + dy) * PW + 2 * p;
                    const float xv[4] = {xr[0], xr[1], xr[2], xr[3]};
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const float4 wa = *reinterpret_cast<const float4*>(cw + wo + (ch * 9 + dy * 3 + dx) * 8);
                        const float4 wb = *reinterpret_cast<const float4*>(cw + wo + (ch * 9 + dy * 3 + dx) * 8 + 4);
                        const float wv[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
                        for (int co = 0; co < 8; ++co) {
                            z0[co] = fmaf(wv[co], xv[dx], z0[co]);
                            z1[co] = fmaf(wv[co], xv[dx + 1], z1[co]);
                        }
                    }
                }
#pragma unroll
            for (int co = 0; co < 8; ++co) {
                const float sc = ca[8 + co], sh = ca[16 + co];
                p1[(co * (T1 + 4) + p + 2) * LQ_RP + h + 2] = fmaxf(fmaxf(fmaf(z0[co], sc, sh), fmaf(z1[co], sc, sh)), 0.0f);
            }
        }
    }
    __syncthreads();

    // ---- 4. conv2 + BN2 + ReLU + pool -> F[t][channel * 44 + row]: thread = (row h, step t), the column pair x eight channels
    float* const F = lds + LQ_L_F;
    {
        const float* ca = cw + LQ_ST_C2A;
#pragma unroll 1
        for (int i = tid; i < LQ_R2 * T2; i += LQ_THREADS) {
            const int t = i / LQ_R2, h = i - t * LQ_R2;
            float z0[8], z1[8];
#pragma unroll
            for (int co = 0; co < 8; ++co) z0[co] = z1[co] = ca[co];
#pragma unroll 1
            for (int ci = 0; ci < 8; ++ci) {
                const float* pr = p1 + (ci * (T1 + 4) + 2 * t) * LQ_RP + h;
                float pv[4][3];
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy) pv[c][dy] = pr[c * LQ_RP + dy];
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const float4 wa = *reinterpret_cast<const float4*>(cw + LQ_ST_C2W + (ci * 9 + dy * 3 + dx) * 8);
                        const float4 wb = *reinterpret_cast<const float4*>(cw + LQ_ST_C2W + (ci * 9 + dy * 3 + dx) * 8 + 4);
                        const float wv[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
                        for (int co = 0; co < 8; ++co) {
                            z0[co] = fmaf(wv[co], pv[dx][dy], z0[co]);
                            z1[co] = fmaf(wv[co], pv[dx + 1][dy], z1[co]);
                        }
                    }
            }
#pragma unroll
            for (int co = 0; co < 8; ++co) {
                const float sc = ca[8 + co], sh = ca[16 + co];
                F[t * LQ_FP + co * LQ_R2 + h] = fmaxf(fmaxf(fmaf(z0[co], sc, sh), fmaf(z1[co], sc, sh)), 0.0f);
            }
        }
    }
    __syncthreads();

    // ---- 5. Gx = F W_ih^T + (b_ih + b_hh), both directions: wave w = column tiles 4 w .. 4 w + 3 of the 48, one or two tiles of
    // sixteen steps.  A lane's outputs: steps 16 mt + 4 (lane >> 4) + r of column 16 nt + (lane & 15).
    {
        f32x4 acc[2][4];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[mt][j] = {0.0f, 0.0f, 0.0f, 0.0f};
        const float* wf = state + LQ_ST_WIH + (size_t)(4 * wave) * (LQ_KS_IH * 64) + lane;
        const float* a0 = F + (lane & 15) * LQ_FP + (lane >> 4);
        if (T2 > 16)      // (workgroup-uniform)
            lq_gemm<4, 2>(acc, wf, LQ_KS_IH, a0, LQ_FP);
        else
            lq_gemm<4, 1>(acc, wf, LQ_KS_IH, a0, LQ_FP);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = 16 * (4 * wave + j) + (lane & 15);
            const float bias = state[LQ_ST_BG + col];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int t = 16 * mt + 4 * (lane >> 4) + r;
                    if (t < T2) gx[t * (2 * LQ_G) + col] = acc[mt][j][r] + bias;
                }
        }
    }
    __syncthreads();      // F is dead from here on

    // ---- 6. the recurrences.  Thread (dir, wave c of six, lane 4 j + g) = gate g (i, f, g, o) of unit 16 c + j.
    float* const hs = lds + LQ_L_HS;      // [step][h_fwd | h_rev]
    float* const hb = lds + LQ_L_HB;      // [parity][dir][96]
    {
        const int dir = wave >= 6 ? 1 : 0;
        const int t384 = tid - dir * LQ_G;
        const int g = lane & 3, u = 16 * (wave - 6 * dir) + (lane >> 2);
        float wB[LQ_H];
        {
            const float4* wp = reinterpret_cast<const float4*>(state + LQ_ST_WHH) + (size_t)dir * (LQ_H / 4) * LQ_G + t384;
#pragma unroll
            for (int q = 0; q < LQ_H / 4; ++q) {
                const float4 v = wp[q * LQ_G];
                wB[4 * q + 0] = v.x;
                wB[4 * q + 1] = v.y;
                wB[4 * q + 2] = v.z;
                wB[4 * q + 3] = v.w;
            }
        }
        // sigmoid(x) = 1 / (1 + 2^(-x log2 e)); the cell-candidate gate is tanh(x) = 2 sigmoid(2x) - 1
        const float kneg = g == 2 ? -2.88539008177792681f : -1.44269504088896341f;
        const float amul = g == 2 ? 2.0f : 1.0f, aadd = g == 2 ? -1.0f : 0.0f;
        const float* gxr = gx + dir * LQ_G + g * LQ_H + u;
        if (tid < 2 * LQ_D) hb[tid] = 0.0f;
        float cst = 0.0f;
        // the input projections of the next three steps are in flight (las_lstm_fwd4_kernel): the loop is unrolled by three so
        // that a slot is a fixed register
        float gq[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int sn = min(d, n - 1), t = dir ? n - 1 - sn : sn;
            gq[d] = gxr[t * (2 * LQ_G)];
        }
        __syncthreads();
        for (int s0 = 0; s0 < n; s0 += 3)
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const int s = s0 + d;
                if (s >= n) break;
                const int t = dir ? n - 1 - s : s;
                const float gc = gq[d];
                {
                    const int sn = min(s + 3, n - 1), tn = dir ? n - 1 - sn : sn;
                    gq[d] = gxr[tn * (2 * LQ_G)];
                }
                const float* hc = hb + (s & 1) * LQ_D + dir * LQ_H;
                float* hn = hb + ((s + 1) & 1) * LQ_D + dir * LQ_H;
                float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int q = 0; q < LQ_H / 4; ++q) {
                    const float4 hv = *reinterpret_cast<const float4*>(hc + 4 * q);
                    a[0] = fmaf(hv.x, wB[4 * q + 0], a[0]);
                    a[1] = fmaf(hv.y, wB[4 * q + 1], a[1]);
                    a[2] = fmaf(hv.z, wB[4 * q + 2], a[2]);
                    a[3] = fmaf(hv.w, wB[4 * q + 3], a[3]);
                }
                const float pre = ((a[0] + a[1]) + (a[2] + a[3])) + gc;
                const float act = fmaf(__builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(kneg * pre)), amul, aadd);
                const float ig = lq_quad_bcast<0>(act), fg = lq_quad_bcast<1>(act), gg = lq_quad_bcast<2>(act), og = lq_quad_bcast<3>(act);
                cst = fmaf(fg, cst, ig * gg);
                const float hv = og * tanhf_(cst);
                if (g == 0) {
                    hn[u] = hv;
                    hs[t * LQ_HP + dir * LQ_H + u] = hv;
                }
                __syncthreads();
            }
    }

    // ---- 7. V = v_proj(h), K = k_proj(h): wave w = column tiles 2 w, 2 w + 1 of the 24 (V's twelve, then K's)
    float* const vk = lds + LQ_L_VK;      // [step][V | K]
    {
        f32x4 acc[2][2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[mt][j] = {0.0f, 0.0f, 0.0f, 0.0f};
        const float* wf = state + LQ_ST_VK + (size_t)(2 * wave) * (LQ_KS_VK * 64) + lane;
        const float* a0 = hs + (lane & 15) * LQ_HP + (lane >> 4);
        if (n > 16)
            lq_gemm<2, 2>(acc, wf, LQ_KS_VK, a0, LQ_HP);
        else
            lq_gemm<2, 1>(acc, wf, LQ_KS_VK, a0, LQ_HP);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = 16 * (2 * wave + j) + (lane & 15);
            const float bias = state[LQ_ST_VKB + col];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int t = 16 * mt + 4 * (lane >> 4) + r;
                    if (t < n) vk[t * LQ_VP + col] = acc[mt][j][r] + bias;
                }
        }
    }
    __syncthreads();

    // ---- 8. attention, wave k = head k (las_attn_fwd_kernel): one pass over the n steps with a running maximum
    float* const ctx = lds + LQ_L_CTX;
    if (wave < LQ_HEADS) {
        const int k = wave;
        const bool on = lane < LQ_HW;
        const int col = LQ_HW * k + (on ? lane : 0);
        const float cvl = on ? state[LQ_ST_CV + 4 * lane + k] : 0.0f;
        float m = -INFINITY, s = 0.0f, acc = 0.0f;
        for (int t = 0; t < n; ++t) {
            const float kk = vk[t * LQ_VP + LQ_D + col];
            const float lg = wave_sum(vk[t * LQ_VP + col] * cvl);
            const float mn = fmaxf(m, lg);
            const float scale = expf(m - mn), p = expf(lg - mn);
            s = fmaf(s, scale, p);
            acc = fmaf(acc, scale, p * kk);
            m = mn;
        }
        if (on) ctx[col] = acc / s;
    }
    __syncthreads();

    // ---- 9. Linear(192,256) - ReLU - Linear(256,C) (las_head_fwd_kernel's order of operations; no dropout)
    float* const y1 = lds + LQ_L_Y1;
    float* const lg = lds + LQ_L_LG;
    if (tid < LQ_HD) {
        float a = state[LQ_ST_B1 + tid];
        const float* w = state + LQ_ST_W1T + tid;
        for (int k = 0; k < LQ_D; ++k) a = fmaf(w[k * LQ_HD], ctx[k], a);
        y1[tid] = fmaxf(a, 0.0f);
    }
    __syncthreads();
    for (int cl = wave; cl < C; cl += LQ_WAVES) {
        float a = 0.0f;
        for (int k = lane; k < LQ_HD; k += 64) a = fmaf(state[LQ_ST_W2 + cl * LQ_HD + k], y1[k], a);
        a = wave_sum(a);
        if (lane == 0) {
            const float v = a + state[LQ_ST_W2 + C * LQ_HD + cl];
            lg[cl] = v;
            if (logits != nullptr) logits[win * C + cl] = v;
        }
    }
    __syncthreads();

    // ---- 10. softmax
    if (tid < C) {
        float mx = lg[0];
        for (int k = 1; k < C; ++k) mx = fmaxf(mx, lg[k]);
        float se = 0.0f;
        for (int k = 0; k < C; ++k) se += expf(lg[k] - mx);
        probs[win * C + tid] = expf(lg[tid] - mx) / se;
    }
}

bool lq_supported(int L, int M, int C) {
    return M == LQ_M && C >= 1 && C <= HOWL_LAS_MAX_LABELS && L >= N_FFT && 1 + L / HOP <= LQ_MAX_FRAMES;
}

}  // namespace

// tests/test_emu_las.py pins the library's `T` exports under howl_las_ to the four functions of howl_hip_las.h.  These entry points
// share that prefix (it is the model's name), so they are exported as weak definitions: the same thing to the dynamic linker and
// to every caller, `W` in the symbol table.
#define LQ_EXPORT __attribute__((weak))

extern "C" {

LQ_EXPORT int howl_las_stream_supported(int L_samples, int M, int C) { return lq_supported(L_samples, M, C) ? 1 : 0; }

LQ_EXPORT size_t howl_las_stream_state_bytes(int C) { return C >= 1 && C <= HOWL_LAS_MAX_LABELS ? lq_state_floats(C) * sizeof(float) : 0; }

LQ_EXPORT size_t howl_las_stream_workspace_bytes(int N, int L_samples) {
    if (N < 1 || N > HOWL_LAS_STREAM_MAX_WINDOWS || !lq_supported(L_samples, LQ_M, 1)) return 0;
    return (size_t)N * (size_t)lq_geom(L_samples).ws_floats * sizeof(float);
}

LQ_EXPORT int howl_las_stream_prepare(const HowlLasParams* prm, const HowlLasBuffers* buffers, int C, void* state, size_t state_bytes,
                            hipStream_t stream) {
    HOWL_REQUIRE(prm && buffers && state, "howl_las_stream_prepare: null pointer");
    HOWL_REQUIRE(C >= 1 && C <= HOWL_LAS_MAX_LABELS, "howl_las_stream_prepare: C=%d unsupported (1..%d)", C, HOWL_LAS_MAX_LABELS);
    HOWL_REQUIRE(state_bytes >= lq_state_floats(C) * sizeof(float), "howl_las_stream_prepare: state of %zu bytes, C=%d needs %zu",
                 state_bytes, C, lq_state_floats(C) * sizeof(float));
    HOWL_REQUIRE((reinterpret_cast<uintptr_t>(state) & 15) == 0, "howl_las_stream_prepare: state must be 16-byte aligned");
    HOWL_REQUIRE(stream_record_complete(prm), "howl_las_stream_prepare: null pointer in HowlLasParams");
    HOWL_REQUIRE(buffers->bn1_mean && buffers->bn1_var && buffers->bn2_mean && buffers->bn2_var,
                 "howl_las_stream_prepare: null pointer in HowlLasBuffers");
    const LqPrep a{*prm, buffers->bn1_mean, buffers->bn1_var, buffers->bn2_mean, buffers->bn2_var};
    const int total = (int)lq_state_floats(C);
    hipLaunchKernelGGL(las_stream_prepare_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, a, C, static_cast<float*>(state));
    HOWL_CHECK_LAUNCH("howl_las_stream_prepare");
    return HOWL_OK;
}

LQ_EXPORT int howl_las_stream_windows(const void* state, const float* pcm, long ld, int N, int L_samples, int frames, const float* fbp, int M,
                            float log_eps, const float* zmuv_pair, int C, float* probs, float* logits, void* ws, size_t ws_bytes,
                            hipStream_t stream) {
    HOWL_REQUIRE(state && pcm && fbp && probs && ws, "howl_las_stream_windows: null pointer");
    HOWL_REQUIRE(lq_supported(L_samples, M, C),
                 "howl_las_stream_windows: L=%d samples, M=%d, C=%d unsupported (M = 40, %d <= L < %d samples, 1 <= C <= %d: "
                 "howl_las_stream_supported)", L_samples, M, C, N_FFT, HOP * LQ_MAX_FRAMES, HOWL_LAS_MAX_LABELS);
    HOWL_STREAM_REQUIRE_GEOMETRY("howl_las_stream_windows", N, HOWL_LAS_STREAM_MAX_WINDOWS, ld, L_samples);
    const LqGeom gm = lq_geom(L_samples);
    HOWL_REQUIRE(frames >= 1 && frames <= gm.T, "howl_las_stream_windows: frames=%d outside 1..%d (T = 1 + L / %d)", frames, gm.T, HOP);
    HOWL_REQUIRE((reinterpret_cast<uintptr_t>(state) & 15) == 0 && (reinterpret_cast<uintptr_t>(ws) & 3) == 0,
                 "howl_las_stream_windows: state must be 16-byte aligned and ws 4-byte aligned");
    const size_t need = (size_t)N * (size_t)gm.ws_floats * sizeof(float);
    if (ws_bytes < need) {
        howl_set_error("howl_las_stream_windows: workspace too small (%zu < %zu bytes)", ws_bytes, need);
        return HOWL_E_WORKSPACE;
    }
    const int nsteps = (((frames + 2) / 2) + 2) / 2;      // <= T2, as frames <= T
    const int aligned = stream_pcm_aligned(pcm, ld, N);
    constexpr size_t lds = (size_t)LQ_LDS_FLOATS * sizeof(float);
    static thread_local size_t granted[16] = {};
    howl_raise_lds(reinterpret_cast<const void*>(las_stream_kernel), lds, granted, "howl_las_stream_windows");
    hipLaunchKernelGGL(las_stream_kernel, dim3((unsigned)N), dim3(LQ_THREADS), lds, stream, static_cast<const float*>(state), pcm, ld,
                       L_samples, nsteps, fbp, log_eps, zmuv_pair, aligned, C, probs, logits, static_cast<float*>(ws));
    HOWL_CHECK_LAUNCH("howl_las_stream_windows");
    return HOWL_OK;
}

}  // extern "C"
