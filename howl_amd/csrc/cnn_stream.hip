// Streaming small-cnn / seq-cnn (include/howl_hip_cnn_stream.h): ONE launch from raw PCM to class probabilities, one workgroup of
// four waves per small-cnn window or per (seq-cnn clip, tile of R = HOWL_CNN_STREAM_TILE_ROWS output rows).  Replaces the chain
// howl_logmel_fwd -> howl_cnn_fwd (cnn_conv0_fwd_kernel, cnn_conv1_fwd_kernel, cnn_head_in_kernel, a GEMM, cnn_head_out_kernel)
// -> softmax: eight launches with the pooled maps, the head's rows and y1 through HBM.  The model is the eval-mode model of cnn.hip
// with its order of operations in both convolutions (the same MFMA tiles, k order and epilogue); the parameters and the running
// statistics are read in place (no prepared state).
//
// One kernel family, cnn_stream_kernel<kind>.  A tile of R output rows [r0, r0 + R) needs conv1 rows [2 r0, 2 r0 + 2 R), pooled
// conv0 rows [4 r0 - 2, 4 r0 + 4 R] (4 R + 3: the slab), conv0 rows [8 r0 - 4, 8 r0 + 8 R + 1] and frames [8 r0 - 14, 8 r0 + 8 R +
// 10] (8 R + 25); small-cnn is the tile r0 = 0, R = 2 of its window (11 pooled rows, all 41 frames).  Per workgroup, with
// workgroup barriers only (nothing is shared between workgroups, so there is no counter, flag or spin loop):
//   1. log-mel + ZMUV of the tile's frames into the frame plane [frame][41] in LDS: logmel_body<4> on a VIEW of the clip that
//      starts tb = max(0, 8 r0 - 20) frames in (200 tb samples; its length and frame count shrink by as much), so that the view's
//      quads 0 .. are the tile's.  The reflect padding at the clip's END is the view's own end; the one at its START would be applied
//      at the view's start, to the view's frames 0 and 1 -- which is why a view that does not start the clip begins a whole quad
//      (frames tb .. tb + 3) in front of the first frame the tile reads (tb + 6): those four rows are computed and never read.
//      Frames in front of the clip and behind its last one are zero rows of the plane (conv0's padding).
//   2. conv0 + bias + MaxPool + ReLU on v_mfma_f32_16x16x4_f32 in passes of eight pooled rows (cnn_conv0_fwd_kernel's tile: the
//      sixteen rows of an MFMA tile are four pooled outputs times the four members of their window, so a lane's four result
//      registers are one window), the weights streamed in chunks of 64 k per pass; eval-mode BN1 applied as the pooled value is
//      stored into conv1's operand slab (48, 4 R + 3, 6 + 4) -- pooled rows outside the CLIP (above row 0, from row Hp on: the
//      odd last conv0 row is dropped there) and the slab's four border columns stay zero: zero AFTER BatchNorm.
//   3. conv1 + bias + MaxPool + ReLU (cnn_conv1_fwd_kernel's tile, 3 R pooled outputs, wave = 16 of the 64 channels, the weights
//      streamed once per workgroup in chunks of 24 k), eval-mode BN2 as the value is stored into the head's rows.
//   4. Linear(192 or 384, 128) + ReLU on the MFMAs (rows x 128, W1 from L2), Linear(128, C) as vector work (eight lanes per
//      (row, class), fixed fold order), max-subtracted softmax, stores.  seq-cnn: the tile's rows behind the clip's last one, up to
//      rows(L_max), are written as zeros; a tile wholly behind it does nothing else.
//
// LDS plan (floats).  Static: logmel_body<4> 60,672 B (37,376 transpose tiles + 5,888 tables + 17,408 filterbank fragments).
// Dynamic, seq-cnn at R = 8 (small-cnn in brackets):
//   frame plane [10 + 8 R + 32][41] 4,346 (48 rows: 1,968) | conv0 weight chunk [64][48] 3,072 | slab [48][4 R + 3][10] 16,800 (5,280)
//   | the two folded BatchNorms 224;   over the plane and the chunk, dead after conv0: conv1's weight chunk [24][80] 1,920 | k ->
//   slab offset 1,200 | head rows [R][196] 1,568 ([1][388]) | y1 [R][132] | logits [R][64]
// = 24,444 floats = 97,776 B dynamic (10,544 floats = 42,176 B), 158,448 of 163,840 B in all.  R = 8 is the largest tile that
// fits (R = 9: 167,440 B); the halo costs 32 computed frames per 8 R used ones (R = 8: 1.5 x the log-mel work, five conv0 passes
// for four passes' worth of rows; R = 4: 2 x, three passes for two), and conv1's 307 KB of weights are read once per R rows.
#include "howl_logmel.hip.h"
#include "howl_stream.hip.h"
#include "../../include/howl_hip_cnn_stream.h"

namespace {

constexpr int CS_NF = 40, CS_XS = CS_NF + 1;      // mel bins; row pitch of the frame plane
constexpr int CS_C1 = 48, CS_C2 = 64;             // channels of the two stages
constexpr int CS_KF = 16;                         // conv0's kernel along frequency
constexpr int CS_WP = 6, CS_W2 = 3;               // pooled columns of the two stages
constexpr int CS_K1 = CS_C1 * 25;                 // conv1's contraction
constexpr int CS_HID = 128;
constexpr int CS_THREADS = 256, CS_WAVES = 4;
constexpr int CS_PN_RS = 10;                      // slab row: 6 columns + 2 zero columns on either side
constexpr int CS_KC1 = 24, CS_WL1 = 80;           // conv1's weight chunk (cnn.hip's)
constexpr int CS_Y1S = CS_HID + 4, CS_LGS = HOWL_CNN_MAX_LABELS;
constexpr float CS_BN_EPS = 1e-5f;
constexpr int CS_SMALL_LO = 5000, CS_SMALL_HI = 8199;
constexpr int CS_SEQ_LO = 800, CS_SEQ_HI = HOP * HOWL_CNN_MAX_FRAMES - 1;

template <int KIND>
struct CsGeom {
    static constexpr bool SEQ = KIND == HOWL_CNN_SEQ;
    static constexpr int KT = SEQ ? 20 : 8, SH = SEQ ? 1 : 2;      // conv0's kernel rows and its stride over the frames
    static constexpr int R = SEQ ? HOWL_CNN_STREAM_TILE_ROWS : 2;  // output rows per workgroup
    static constexpr int PROWS = 4 * R + 3;                        // pooled conv0 rows of the slab
    static constexpr int PASSES = (PROWS + 7) / 8;                 // conv0 passes of eight pooled rows
    static constexpr int MT = (3 * R + 3) / 4;                     // conv1's MFMA row tiles: 3 R pooled outputs, four per tile
    static constexpr int PADF = KT / 2;                            // zero rows in front of the plane (frames in front of the clip)
    static constexpr int FCAP = SEQ ? 8 * R + 32 : 44;             // frames the frontend may store
    static constexpr int FROWS = PADF + FCAP;
    static constexpr int F = SEQ ? CS_C2 * CS_W2 : CS_C2 * 2 * CS_W2;
    static constexpr int XHS = F + 4;                              // head rows: A fragments of sixteen rows on distinct banks
    static constexpr int HR = SEQ ? R : 1;                         // head rows per workgroup
    static constexpr int PN_CS = PROWS * CS_PN_RS;
    // dynamic LDS, in floats
    static constexpr int L_FB = 0;
    static constexpr int L_WL0 = (FROWS * CS_XS + 3) / 4 * 4;
    static constexpr int L_PN = L_WL0 + 64 * CS_C1;
    static constexpr int L_BN = L_PN + CS_C1 * PN_CS;
    static constexpr int FLOATS = L_BN + 2 * CS_C1 + 2 * CS_C2;
    // over the plane and conv0's chunk
    static constexpr int L_WL1 = 0;
    static constexpr int L_KOFF = L_WL1 + CS_KC1 * CS_WL1;
    static constexpr int L_XH = L_KOFF + CS_K1;
    static constexpr int L_Y1 = L_XH + HR * XHS;
    static constexpr int L_LG = L_Y1 + HR * CS_Y1S;
    static_assert(L_LG + HR * CS_LGS <= L_PN, "conv1's and the head's buffers lie over the frame plane and conv0's chunk only");
    static_assert(MT * 4 >= 3 * R && R <= 16 && HR <= 16, "one 16-row MFMA tile of head rows");
};

struct CsArgs {
    HowlCnnParams p;
    const float *m1, *v1, *m2, *v2;      // running mean and variance of BN1 (48) and BN2 (64)
    const float* pcm;
    long ld;
    int L_max, rows_max;
    const long long* n_samples;
    const float* fbp;
    float log_eps;
    const float* zmuv;
    int C;
    float *probs, *logits;
    long out_ld;
};

__host__ __device__ inline int cs_rows(int kind, int L) {
    if (kind == HOWL_CNN_SMALL) return (L >= CS_SMALL_LO && L <= CS_SMALL_HI) ? 2 : 0;
    if (kind != HOWL_CNN_SEQ || L < CS_SEQ_LO || L > CS_SEQ_HI) return 0;
    const int T = 1 + L / HOP;
    return ((((T + 1) / 2 - 1) / 2 + 1) / 2);
}

// the maximum of a pool window, then the ReLU (cnn.hip's pool_relu without the choice)
__device__ __forceinline__ float cs_pool_relu(const f32x4& a, float bias) {
    float best = a[0] + bias;
#pragma unroll
    for (int r = 1; r < 4; ++r) {
        const float v = a[r] + bias;
        best = v > best ? v : best;
    }
    return fmaxf(best, 0.0f);
}

template <int KIND>
__global__ __launch_bounds__(CS_THREADS) void cnn_stream_kernel(CsArgs a) {
    using G = CsGeom<KIND>;
    constexpr int KT = G::KT, SH = G::SH, R = G::R, K0 = KT * CS_KF;
    HIP_DYNAMIC_SHARED(float, lds)
    const HowlCnnParams& p = a.p;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = G::SEQ ? blockIdx.y : blockIdx.x;      // window / clip
    const int r0 = G::SEQ ? (int)blockIdx.x * R : 0;     // the tile's first output row
    const int C = a.C;

    // the clip's own geometry (workgroup-uniform)
    int L = a.L_max;
    if (G::SEQ && a.n_samples != nullptr) {
        const long long ns = a.n_samples[n];
        L = (int)(ns < CS_SEQ_LO ? CS_SEQ_LO : (ns > a.L_max ? a.L_max : ns));
    }
    const int T = 1 + L / HOP;
    const int H0 = G::SEQ ? T + 1 : T / 2 + 1, Hp = H0 / 2;      // conv0's rows; pooled rows (the odd last row is dropped)
    const int H2 = G::SEQ ? ((Hp - 1) / 2 + 1) / 2 : 2;          // output rows
    const int nrows = min(R, H2 - r0);                           // this tile's
    float* const out_p = a.probs + (long)n * a.out_ld;
    float* const out_l = a.logits != nullptr ? a.logits + (long)n * a.out_ld : nullptr;
    if (G::SEQ) {
        // rows behind the clip's last one, up to the launch's rows(L_max): zeros
        const int z0 = max(r0, H2), z1 = min(r0 + R, a.rows_max);
        for (int e = z0 * C + tid; e < z1 * C; e += CS_THREADS) {
            out_p[e] = 0.0f;
            if (out_l != nullptr) out_l[e] = 0.0f;
        }
        if (nrows <= 0) return;      // (workgroup-uniform, in front of the first barrier)
    }

    float* const fb = lds + G::L_FB;
    float* const wl0 = lds + G::L_WL0;
    float* const pn = lds + G::L_PN;
    float* const sc1 = lds + G::L_BN;
    float* const sh1 = sc1 + CS_C1;
    float* const sc2 = sh1 + CS_C1;
    float* const sh2 = sc2 + CS_C2;

    // what later phases read without having written it: frames outside the clip, the slab's borders; the folded BatchNorms
    for (int i = tid; i < G::L_WL0; i += CS_THREADS) fb[i] = 0.0f;
    for (int i = tid; i < CS_C1 * G::PN_CS; i += CS_THREADS) pn[i] = 0.0f;
    if (tid < CS_C1) {
        // y = z * sc + sh (cnn.hip's bn_affine from the running statistics)
        const float sc = p.bn1_w[tid] * (1.0f / sqrtf(a.v1[tid] + CS_BN_EPS));
        sc1[tid] = sc;
        sh1[tid] = p.bn1_b[tid] - a.m1[tid] * sc;
    } else if (tid >= 64 && tid < 64 + CS_C2) {
        const int c = tid - 64;
        const float sc = p.bn2_w[c] * (1.0f / sqrtf(a.v2[c] + CS_BN_EPS));
        sc2[c] = sc;
        sh2[c] = p.bn2_b[c] - a.m2[c] * sc;
    }

    // ---- 1. log-mels (+ ZMUV) of the tile's frames: view frame i = clip frame tb + i -> fb[(PADF + i) * 41 + mel]
    const int tb = G::SEQ ? max(0, 8 * r0 - 20) : 0;
    {
        const float* view = a.pcm + (long)n * a.ld + (long)HOP * tb;
        const int Lv = L - HOP * tb, Tv = T - tb, nv = min(Tv, G::FCAP);
        const int aligned = (reinterpret_cast<uintptr_t>(view) & 7) == 0 ? 1 : 0;
        // (the body's one workgroup barrier covers the stores above)
        logmel_body<CS_WAVES, NG_BANDED>(view, Lv, 0, Tv, nv, a.fbp, CS_NF, a.log_eps, a.zmuv, fb + G::PADF * CS_XS, 1, (nv + QUAD - 1) / QUAD,
                                         aligned, 0u, 1u, CS_XS);
    }
    __syncthreads();

    // ---- 2. conv0 + bias + pool + ReLU, BN1 -> the slab: row j = pooled row hp_base + j
    const int hp_base = 4 * r0 - 2;
    const int kk = lane >> 4;
    // conv0's weight chunks come one chunk ahead through registers: the loads of chunk ch + 1 (the next pass starts over at 0) are in
    // flight under the MFMAs of chunk ch.  One workgroup per compute unit has nobody else to hide an L2 round trip behind.
    constexpr int NCH0 = K0 / 64, E0 = 64 * CS_C1 / CS_THREADS;
    float nx0[E0];
#pragma unroll
    for (int e = 0; e < E0; ++e) {
        const int i = tid + CS_THREADS * e;
        nx0[e] = p.conv0_w[(i >> 6) * K0 + (i & 63)];
    }
#pragma unroll 1
    for (int ps = 0; ps < G::PASSES; ++ps) {
        const int hp0 = hp_base + 8 * ps;
        if (hp0 >= Hp || hp0 + 8 <= 0) continue;      // (workgroup-uniform) no pooled row of the pass is inside the clip
        int abase[3];
#pragma unroll
        for (int mt = 0; mt < 3; ++mt) {
            const int i = lane & 15, pp = (wave * 3 + mt) * 4 + (i >> 2);
            const int hl = 2 * (pp / CS_WP) + ((i >> 1) & 1), w0 = 2 * (pp % CS_WP) + (i & 1);
            // plane row of the conv0 row's first frame; rows whose pooled row is outside the slab or the clip are computed on
            // rows of the plane that exist and dropped below
            int fr = (2 * hp0 + hl) * SH - KT / 2 - tb + G::PADF;
            fr = fr < 0 ? 0 : (fr > G::FROWS - KT ? G::FROWS - KT : fr);
            abase[mt] = fr * CS_XS + 2 * w0 + kk;
        }
        f32x4 acc[3][3];
#pragma unroll
        for (int mt = 0; mt < 3; ++mt)
#pragma unroll
            for (int nt = 0; nt < 3; ++nt) acc[mt][nt] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int ch = 0; ch < NCH0; ++ch) {
            __syncthreads();
            const int nch = ch + 1 < NCH0 ? ch + 1 : 0;
#pragma unroll
            for (int e = 0; e < E0; ++e) {
                const int i = tid + CS_THREADS * e, c = i >> 6, kc = i & 63;
                wl0[kc * CS_C1 + c] = nx0[e];
                nx0[e] = p.conv0_w[c * K0 + 64 * nch + kc];
            }
            __syncthreads();
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
                const int S = 16 * ch + s;
                const int off = (S >> 2) * CS_XS + (S & 3) * 4;
                float bv[3], av[3];
#pragma unroll
                for (int nt = 0; nt < 3; ++nt) bv[nt] = wl0[(4 * s + kk) * CS_C1 + nt * 16 + (lane & 15)];
#pragma unroll
                for (int mt = 0; mt < 3; ++mt) av[mt] = fb[abase[mt] + off];
#pragma unroll
                for (int mt = 0; mt < 3; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 3; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int mt = 0; mt < 3; ++mt) {
            const int pp = (wave * 3 + mt) * 4 + (lane >> 4);
            const int j = 8 * ps + pp / CS_WP, wp = pp % CS_WP, hp = hp_base + j;
            const bool valid = j < G::PROWS && hp >= 0 && hp < Hp;
#pragma unroll
            for (int nt = 0; nt < 3; ++nt) {
                const int c = nt * 16 + (lane & 15);
                const float v = cs_pool_relu(acc[mt][nt], p.conv0_b[c]);
                if (valid) pn[c * G::PN_CS + j * CS_PN_RS + 2 + wp] = fmaf(v, sc1[c], sh1[c]);
            }
        }
    }
    __syncthreads();      // the slab is complete; the plane and conv0's chunk are dead from here on

    // ---- 3. conv1 + bias + pool + ReLU, BN2 -> the head's rows
    float* const wl1 = lds + G::L_WL1;
    int* const koff = reinterpret_cast<int*>(lds + G::L_KOFF);
    float* const xh = lds + G::L_XH;
    float* const y1 = lds + G::L_Y1;
    float* const lg = lds + G::L_LG;
    for (int i = tid; i < CS_K1; i += CS_THREADS) {
        const int ci = i / 25, r = i - ci * 25;
        koff[i] = ci * G::PN_CS + (r / 5) * CS_PN_RS + r % 5;
    }
    for (int i = tid; i < G::HR * G::XHS; i += CS_THREADS) xh[i] = 0.0f;
    {
        const int co = wave * 16 + (lane & 15);
        int abase[G::MT];
#pragma unroll
        for (int mt = 0; mt < G::MT; ++mt) {
            const int i = lane & 15, pp = min(mt * 4 + (i >> 2), 3 * R - 1);      // (outputs behind the tile's last: any address inside)
            const int h1l = 2 * (pp / CS_W2) + ((i >> 1) & 1), w1 = 2 * (pp % CS_W2) + (i & 1);
            abase[mt] = 2 * h1l * CS_PN_RS + w1;
        }
        f32x4 acc[G::MT];
#pragma unroll
        for (int mt = 0; mt < G::MT; ++mt) acc[mt] = {0.0f, 0.0f, 0.0f, 0.0f};
        // conv1's weight chunks come D1 chunks ahead through a ring of registers (a chunk's MFMAs are a quarter of an L2 round trip)
        constexpr int NCH1 = CS_K1 / CS_KC1, D1 = 5, E1 = CS_KC1 * CS_C2 / CS_THREADS;
        static_assert(NCH1 % D1 == 0 && E1 * CS_THREADS == CS_KC1 * CS_C2, "whole rings of whole chunks");
        int src[E1], dst[E1];
#pragma unroll
        for (int e = 0; e < E1; ++e) {
            const int i = tid + CS_THREADS * e, c = i / CS_KC1, kc = i - c * CS_KC1;
            src[e] = c * CS_K1 + kc;
            dst[e] = kc * CS_WL1 + c;
        }
        float nx1[D1][E1];
#pragma unroll
        for (int j = 0; j < D1; ++j)
#pragma unroll
            for (int e = 0; e < E1; ++e) nx1[j][e] = p.conv1_w[src[e] + CS_KC1 * j];
#pragma unroll 1
        for (int ch0 = 0; ch0 < NCH1; ch0 += D1) {
#pragma unroll
            for (int j = 0; j < D1; ++j) {
                const int ch = ch0 + j;
                __syncthreads();
#pragma unroll
                for (int e = 0; e < E1; ++e) wl1[dst[e]] = nx1[j][e];
                if (ch + D1 < NCH1) {      // (workgroup-uniform)
#pragma unroll
                    for (int e = 0; e < E1; ++e) nx1[j][e] = p.conv1_w[src[e] + CS_KC1 * (ch + D1)];
                }
                __syncthreads();
#pragma unroll
                for (int s = 0; s < CS_KC1 / 4; ++s) {
                    const int ko = koff[CS_KC1 * ch + 4 * s + kk];
                    const float bv = wl1[(4 * s + kk) * CS_WL1 + co];
#pragma unroll
                    for (int mt = 0; mt < G::MT; ++mt)
                        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pn[abase[mt] + ko], bv, acc[mt], 0, 0, 0);
                }
            }
        }
        const float b = p.conv1_b[co], s2 = sc2[co], t2 = sh2[co];
#pragma unroll
        for (int mt = 0; mt < G::MT; ++mt) {
            const int pp = mt * 4 + (lane >> 4);
            if (pp < 3 * R) {
                const float v = fmaf(cs_pool_relu(acc[mt], b), s2, t2);
                // seq-cnn flattens (c, w) into the row of output row pp / 3, small-cnn (c, h, w) into the window's one row
                if (G::SEQ) xh[(pp / CS_W2) * G::XHS + co * CS_W2 + pp % CS_W2] = v;
                else xh[co * (2 * CS_W2) + pp] = v;
            }
        }
    }
    __syncthreads();

    // ---- 4. y1 = relu(Xh W1^T + b1): one 16-row MFMA tile (rows behind HR repeat the last one and are dropped), wave = 32 units
    {
        const int nn = lane & 15;
        const float* ap = xh + min(nn, G::HR - 1) * G::XHS + kk;
        const float* w1a = p.w1 + (size_t)(wave * 32 + nn) * G::F + kk;
        const float* w1b = w1a + (size_t)16 * G::F;
        f32x4 h0 = {0.0f, 0.0f, 0.0f, 0.0f}, h1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 24
        for (int s = 0; s < G::F / 4; ++s) {      // (24 steps' loads of W1 in flight at a time)
            const float av = ap[4 * s];
            h0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w1a[4 * s], h0, 0, 0, 0);
            h1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w1b[4 * s], h1, 0, 0, 0);
        }
        const float b1a = p.b1[wave * 32 + nn], b1b = p.b1[wave * 32 + 16 + nn];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * kk + r;
            if (row < G::HR) {
                y1[row * CS_Y1S + wave * 32 + nn] = fmaxf(h0[r] + b1a, 0.0f);
                y1[row * CS_Y1S + wave * 32 + 16 + nn] = fmaxf(h1[r] + b1b, 0.0f);
            }
        }
    }
    __syncthreads();
    // logits[row][cls] = b2[cls] + sum_k y1[row][k] W2[cls][k]: eight lanes per output (k = part + 8 i), folded in a fixed order
    const int nout = (G::SEQ ? nrows : 1) * C;
    for (int ob = 0; ob < nout; ob += CS_THREADS / 8) {
        const int o = min(ob + (tid >> 3), nout - 1), part = tid & 7;
        const int row = o / C, cls = o - row * C;
        const float* yr = y1 + row * CS_Y1S + part;
        const float* wr = p.w2 + (size_t)cls * CS_HID + part;
        float s = 0.0f;
#pragma unroll 8
        for (int i = 0; i < CS_HID / 8; ++i) s = fmaf(yr[8 * i], wr[8 * i], s);
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        if (part == 0) lg[row * CS_LGS + cls] = s + p.b2[cls];
    }
    __syncthreads();
    // softmax
    for (int e = tid; e < nout; e += CS_THREADS) {
        const int row = e / C, cls = e - row * C;
        const float* l = lg + row * CS_LGS;
        float mx = l[0];
        for (int k = 1; k < C; ++k) mx = fmaxf(mx, l[k]);
        float se = 0.0f;
        for (int k = 0; k < C; ++k) se += expf(l[k] - mx);
        const long d = (long)(r0 + row) * C + cls;
        out_p[d] = expf(l[cls] - mx) / se;
        if (out_l != nullptr) out_l[d] = l[cls];
    }
}

bool cs_supported(int kind, int L, int M, int C) {
    return M == CS_NF && C >= 1 && C <= HOWL_CNN_MAX_LABELS && cs_rows(kind, L) > 0;
}

constexpr size_t CS_WS_BYTES = 16;      // nothing goes through the workspace

template <int KIND>
int cs_launch(const char* name, const CsArgs& a, int N, hipStream_t stream) {
    using G = CsGeom<KIND>;
    constexpr size_t lds = (size_t)G::FLOATS * sizeof(float);
    static thread_local size_t granted[16] = {};
    howl_raise_lds(reinterpret_cast<const void*>(cnn_stream_kernel<KIND>), lds, granted, name);
    const dim3 grid = G::SEQ ? dim3((unsigned)((a.rows_max + G::R - 1) / G::R), (unsigned)N) : dim3((unsigned)N);
    hipLaunchKernelGGL(cnn_stream_kernel<KIND>, grid, dim3(CS_THREADS), lds, stream, a);
    HOWL_CHECK_LAUNCH(name);
    return HOWL_OK;
}

}  // namespace

// tests/test_emu_cnn.py pins the library's `T` exports under howl_cnn_ to the five functions of howl_hip_cnn.h.  These entry points
// share that prefix (it is the models' name), so they are exported as weak definitions, as gru_stream.hip and las_stream.hip export
// their own: the same thing to the dynamic linker and to every caller, `W` in the symbol table.
#define CS_EXPORT __attribute__((weak))

// what both launches refuse, in one order
#define CS_REQUIRE_COMMON(name, kind, L)                                                                                               \
    do {                                                                                                                               \
        HOWL_REQUIRE(prm && buffers && pcm && fbp && probs && ws, name ": null pointer");                                               \
        HOWL_REQUIRE(stream_record_complete(prm), name ": null pointer in HowlCnnParams");                                              \
        HOWL_REQUIRE(buffers->bn1_mean && buffers->bn1_var && buffers->bn2_mean && buffers->bn2_var,                                    \
                     name ": null pointer in HowlCnnBuffers");                                                                          \
        HOWL_REQUIRE(cs_supported(kind, L, M, C),                                                                                       \
                     name ": L=%d samples, M=%d, C=%d unsupported (M = 40, %d <= L <= %d samples, 1 <= C <= %d: "                       \
                          "howl_cnn_stream_supported)", L, M, C, kind == HOWL_CNN_SMALL ? CS_SMALL_LO : CS_SEQ_LO,                      \
                     kind == HOWL_CNN_SMALL ? CS_SMALL_HI : CS_SEQ_HI, HOWL_CNN_MAX_LABELS);                                            \
    } while (0)

#define CS_REQUIRE_WORKSPACE(name)                                                                                  \
    do {                                                                                                            \
        if (ws_bytes < CS_WS_BYTES) {                                                                               \
            howl_set_error(name ": workspace too small (%zu < %zu bytes)", ws_bytes, CS_WS_BYTES);                   \
            return HOWL_E_WORKSPACE;                                                                                \
        }                                                                                                           \
    } while (0)

extern "C" {

CS_EXPORT int howl_cnn_stream_supported(int kind, int L_samples, int M, int C) { return cs_supported(kind, L_samples, M, C) ? 1 : 0; }

CS_EXPORT size_t howl_cnn_stream_workspace_bytes(int kind, int N, int L_max) {
    if (N < 1 || N > HOWL_CNN_STREAM_MAX_WINDOWS || cs_rows(kind, L_max) == 0) return 0;
    return CS_WS_BYTES;
}

CS_EXPORT size_t howl_cnn_stream_rows(int kind, int L_samples) { return (size_t)cs_rows(kind, L_samples); }

CS_EXPORT int howl_cnn_stream_windows(const HowlCnnParams* prm, const HowlCnnBuffers* buffers, const float* pcm, long ld, int N,
                                      int L_samples, const float* fbp, int M, float log_eps, const float* zmuv_pair, int C, float* probs,
                                      float* logits, void* ws, size_t ws_bytes, hipStream_t stream) {
    CS_REQUIRE_COMMON("howl_cnn_stream_windows", HOWL_CNN_SMALL, L_samples);
    HOWL_STREAM_REQUIRE_GEOMETRY("howl_cnn_stream_windows", N, HOWL_CNN_STREAM_MAX_WINDOWS, ld, L_samples);
    CS_REQUIRE_WORKSPACE("howl_cnn_stream_windows");
    const CsArgs a{*prm, buffers->bn1_mean, buffers->bn1_var, buffers->bn2_mean, buffers->bn2_var, pcm, ld, L_samples, 2, nullptr, fbp,
                   log_eps, zmuv_pair, C, probs, logits, (long)C};
    return cs_launch<HOWL_CNN_SMALL>("howl_cnn_stream_windows", a, N, stream);
}

CS_EXPORT int howl_cnn_stream_clips(const HowlCnnParams* prm, const HowlCnnBuffers* buffers, const float* pcm, long ld, int N, int L_max,
                                    const long long* n_samples, const float* fbp, int M, float log_eps, const float* zmuv_pair, int C,
                                    float* probs, float* logits, long out_ld, void* ws, size_t ws_bytes, hipStream_t stream) {
    CS_REQUIRE_COMMON("howl_cnn_stream_clips", HOWL_CNN_SEQ, L_max);
    HOWL_REQUIRE(N >= 1 && N <= HOWL_CNN_STREAM_MAX_WINDOWS, "howl_cnn_stream_clips: N=%d clips unsupported (1..%d)", N,
                 HOWL_CNN_STREAM_MAX_WINDOWS);
    HOWL_REQUIRE(ld >= 0, "howl_cnn_stream_clips: negative clip stride %ld", ld);
    const int rows_max = cs_rows(HOWL_CNN_SEQ, L_max);
    HOWL_REQUIRE(out_ld >= (long)rows_max * C, "howl_cnn_stream_clips: out_ld=%ld floats per clip, this call writes %ld", out_ld,
                 (long)rows_max * C);
    CS_REQUIRE_WORKSPACE("howl_cnn_stream_clips");
    const CsArgs a{*prm, buffers->bn1_mean, buffers->bn1_var, buffers->bn2_mean, buffers->bn2_var, pcm, ld, L_max, rows_max, n_samples, fbp,
                   log_eps, zmuv_pair, C, probs, logits, out_ld};
    return cs_launch<HOWL_CNN_SEQ>("howl_cnn_stream_clips", a, N, stream);
}

}  // extern "C"
