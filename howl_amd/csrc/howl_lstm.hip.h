// Device helpers of the four-sequence LSTM recurrence step (v_mfma_f32_4x4x1 with block broadcast, the in-quad transpose, the gate
// nonlinearities), shared by lstm.hip (lstm_fwd4_kernel / lstm_bwd4_kernel) and lstm_stream.hip.  Moved out of lstm.hip verbatim.
#pragma once
#include "howl_common.hip.h"

namespace {

// Gate nonlinearities on the hardware exp2 / reciprocal (1 ulp each): the cell update sits on the critical path of every
// one of the 38-81 sequential steps, and the library expf / tanhf / division cost ~10x the instructions.  Absolute error
// ~1e-7, far inside the 2e-6 the parity tests hold the hidden states to.
__device__ __forceinline__ float sigmoidf_(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
}
__device__ __forceinline__ float tanhf_(float x) {
    // no clamp needed: 2^(+big) = inf -> rcp 0 -> 1; 2^(-big) = 0 -> rcp 1 -> -1 (v_exp_f32 / v_rcp_f32 saturate cleanly)
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(2.88539008177792681f * x));
}

// The A operand of the four-sequence recurrences is the same for all sixteen blocks of v_mfma_f32_4x4x1_16b_f32 (the four
// sequences' h or dG values of one k).  With cbsz = 4 the instruction takes A from the lanes of ONE block (abid) for all
// sixteen, so a lane (block J, row i) loads only the four k values 4J..4J+3 of its row -- one 16-byte LDS read per wave and
// step instead of sixteen (which was as much LDS-pipe time per step, 256 x 1 KB, as the step's matrix work) -- and the
// sixty-four instructions walk abid over the blocks.  acc[e] is the chain of k = e mod 4.
template <int J, int OFF, int N, int JEND = 16>
__device__ __forceinline__ void bcast_mfma64(const float4& a, const float (&w)[N], f32x4 (&acc)[4]) {
    acc[0] = __builtin_amdgcn_mfma_f32_4x4x1f32(a.x, w[OFF + 4 * J + 0], acc[0], 4, J, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_4x4x1f32(a.y, w[OFF + 4 * J + 1], acc[1], 4, J, 0);
    acc[2] = __builtin_amdgcn_mfma_f32_4x4x1f32(a.z, w[OFF + 4 * J + 2], acc[2], 4, J, 0);
    acc[3] = __builtin_amdgcn_mfma_f32_4x4x1f32(a.w, w[OFF + 4 * J + 3], acc[3], 4, J, 0);
    if constexpr (J + 1 < JEND) bcast_mfma64<J + 1, OFF, N, JEND>(a, w, acc);
}
// 4 x 4 transpose inside every quad of lanes: v[r] of lane 4q + l  <->  v[l] of lane 4q + r.  Two butterfly stages: the
// partner's registers arrive by v_mov_b32_dpp quad_perm, a select on the lane's parity keeps or takes (16 instructions; a DPP
// bank mask cannot do the select: its banks are whole quads).
__device__ __forceinline__ void quad_transpose(float (&v)[4], bool bit0, bool bit1) {
    auto xor1 = [](float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xf, 0xf, true)); };
    auto xor2 = [](float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xf, 0xf, true)); };
    // stage 1: lane bit 0 <-> register bit 0: even lanes take the partner's v[0] as v[1], odd lanes its v[1] as v[0]
    {
        const float p0 = xor1(v[0]), p1 = xor1(v[1]), p2 = xor1(v[2]), p3 = xor1(v[3]);
        v[0] = bit0 ? p1 : v[0];
        v[1] = bit0 ? v[1] : p0;
        v[2] = bit0 ? p3 : v[2];
        v[3] = bit0 ? v[3] : p2;
    }
    // stage 2: lane bit 1 <-> register bit 1
    {
        const float p0 = xor2(v[0]), p1 = xor2(v[1]), p2 = xor2(v[2]), p3 = xor2(v[3]);
        v[0] = bit1 ? p2 : v[0];
        v[2] = bit1 ? v[2] : p0;
        v[1] = bit1 ? p3 : v[1];
        v[3] = bit1 ? v[3] : p1;
    }
}

}  // namespace
