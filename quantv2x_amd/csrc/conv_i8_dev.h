// Device helpers the int8 convolution kernels share (conv_i8*.hip, conv1x1_i8.hip, gconv3x3_i8.hip, bottleneck_i8.hip).  Each is used only
// where the kernel compiles to the instructions it had with the text written out; the sites that did not are left as they were.
#pragma once
#include "common.h"

namespace qv2x {

// a compile-time int as a function argument (generic lambdas take their unroll index, tap or register number this way)
template <int V> struct IC { static constexpr int value = V; };

// index of pixel (y, x) of image `img` in a padded [n][h + 2][w + 2][channels] BEV tensor, as a T (the integer type the address needs).
// A macro: as an inlined function the same expression moved instructions in every kernel that used it.
#define QV2X_BEV_PIXEL(T, img, y, x, h, w) ((T)((img) * ((h) + 2) + (y) + 1) * ((w) + 2) + (x) + 1)

// s + the sum of the 16 (code - 128) bytes of v
__device__ __forceinline__ int sum16(v4i v, int s = 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) s = __builtin_amdgcn_sdot4(v[q], 0x01010101, s, false);
    return s;
}
// a quad of lanes holds the four 16-byte pieces of one 64-channel pixel: the pixel's channel sum, in all four
__device__ __forceinline__ int quad_sum64(v4i v) {
    int s = sum16(v);
    s += __builtin_amdgcn_mov_dpp(s, 0xB1, 0xf, 0xf, false);          // quad_perm [1,0,3,2]
    s += __builtin_amdgcn_mov_dpp(s, 0x4E, 0xf, 0xf, false);          // quad_perm [2,3,0,1]
    return s;
}

// The weights-as-A-operand epilogues leave a lane with four packed channel quads of its pixel: 0-3 | 8-11 | 16-19 | 24-27 in the lower
// half-wave, +4 in the upper.  The half-wave exchange v_permlane32_swap turns them into 16 contiguous channels -- lower half 0-15, upper
// half 16-31 of the same pixel -- for one 16-byte store, without LDS staging.
__device__ __forceinline__ v4i gather16(const int (&pk)[4]) {
    const auto s02 = __builtin_amdgcn_permlane32_swap(pk[0], pk[2], false, false);
    const auto s13 = __builtin_amdgcn_permlane32_swap(pk[1], pk[3], false, false);
    v4i ob;
    ob[0] = s02[0]; ob[1] = s02[1]; ob[2] = s13[0]; ob[3] = s13[1];
    return ob;
}

// ONE output of the weights-stationary kernels' woven epilogue (conv_i8_ws.hip, conv_i8_ws2.hip): register R of the pending accumulator
// = channel 8 (R >> 2) + 4 half + (R & 3) of the lane's pixel.  `sum` already holds the channel's correction term (the first MFMA's C
// operand), `tot` is the pixel's window sum.  Every fourth call closes a group of four codes into pk[R >> 2].
template <int R>
__device__ __forceinline__ void ws_requant(int sum, int aw, int tot, float bias, float scale, float rd, float zp, float qlow, unsigned& qa, int (&pk)[4]) {
    const float y = bias + (float)(__mul24(aw, tot) + sum) * scale;
    if ((R & 3) == 0) qa = 0;
    q_add(y, R & 3, rd, zp, qlow, qa);                                // (common.h: fma + v_cvt_pk_u8_f32, two instructions per output)
    if ((R & 3) == 3) pk[R >> 2] = (int)(qa ^ 0x80808080u);
}

}  // namespace qv2x
