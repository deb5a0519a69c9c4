// Camera encoder, back end: depth_head (cin -> D) and image_head (cin -> C) of QuantCamEncode_Resnet101 (opencood/quant/quant_block.py:
// 744-860), two 1x1 QuantModules on the trunk's codes, each with its own activation quantizer and NO ReLU in front of it -- so the zero
// point sits anywhere in 0..255 -- written dequantized, as the f32 [views][D | C][fH][fW] tensors the lift-splat reads.
//
// GEMM view as conv1x1_i8.hip: rows = output channels (the weights are the A operand of v_mfma_i32_32x32x32_i8), columns = pixels,
// K = cin.  The rows of BOTH heads form one list (each head padded to a multiple of 32 on the host), so one launch serves both and a wave
// reads its 32 pixels once from memory (again from L1 for every further 32-row tile).  One wave = 32 pixels x all row tiles; a lane ends
// up with one pixel and 16 rows per tile: the zero-point correction uses the lane's own window sum, and for a fixed row the 32 lanes
// of a half-wave store 32 consecutive floats of the channel-major output.  The feature map of a camera is small (48 x 64 at the OPV2V
// shape): the launch is bound by its latency, not by the matrix pipe -- DESIGN.md section 14.
#include "common.h"

namespace qv2x {
namespace {

struct HeadsArgs {
    const int8_t* in; const int8_t* w; const float* scale; const int32_t* corr; const int32_t* aw; const float* bias;
    float* depth; float* feats;
    int views, h, wd, cin, ks, D, C, dp, tiles_r, M;
    float d_delta, d_rdelta, d_zp, f_delta, f_rdelta, f_zp;
};

__global__ __launch_bounds__(256) void cam_heads_kernel(const HeadsArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int tile = blockIdx.x * 4 + wave;
    if (tile * 32 >= a.M) return;
    const int m = tile * 32 + l31;
    const bool valid = m < a.M;
    const int mm = valid ? m : a.M - 1;
    const int hw = a.h * a.wd;
    const int img = mm / hw, rem = mm - img * hw;
    const int y0 = rem / a.wd, x0 = rem - y0 * a.wd;
    const int8_t* src = a.in + ((size_t)(img * (a.h + 2) + y0 + 1) * (a.wd + 2) + x0 + 1) * a.cin + 16 * half;
    int xs = 0;
    for (int ks = 0; ks < a.ks; ++ks) {
        const v4i fb = *(const v4i*)(src + 32 * ks);
#pragma unroll
        for (int q = 0; q < 4; ++q) xs = __builtin_amdgcn_sdot4(fb[q], 0x01010101, xs, false);
    }
    const int tot = xs + __shfl_xor(xs, 32);                           // sum of the pixel's (code - 128) over cin
    for (int rt = 0; rt < a.tiles_r; ++rt) {
        const int8_t* wsrc = a.w + ((size_t)rt * a.ks) * 1024 + lane * 16;
        v16i acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0;
        for (int ks = 0; ks < a.ks; ++ks) {
            const v4i fa = *(const v4i*)(wsrc + (size_t)ks * 1024);
            const v4i fb = *(const v4i*)(src + 32 * ks);
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb, acc, 0, 0, 0);
        }
        const bool is_depth = rt * 32 < a.dp;                          // wave-uniform
        const int row0 = is_depth ? rt * 32 : rt * 32 - a.dp;          // first row of the tile inside its head
        const int nrows = is_depth ? a.D : a.C;
        float* dst = (is_depth ? a.depth : a.feats) + ((size_t)img * nrows) * hw + rem;
        const float delta = is_depth ? a.d_delta : a.f_delta, rd = is_depth ? a.d_rdelta : a.f_rdelta, zp = is_depth ? a.d_zp : a.f_zp;
        const int izp = (int)zp;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = mfma32_row(r, lane), ch = rt * 32 + rl;     // row in the tile, row in the joint list
            const int T = acc[r] + a.aw[ch] * tot + a.corr[ch];
            const float y = a.bias[ch] + (float)T * a.scale[ch];
            const float code = fminf(fmaxf(rintf(__builtin_fmaf(y, rd, zp)), 0.0f), 255.0f);
            // code - zp as integers: a code of -0 (rint of a small negative value) must give +0, as the integer code 0 does
            if (valid && row0 + rl < nrows) dst[(size_t)(row0 + rl) * hw] = (float)((int)code - izp) * delta;
        }
    }
}

}  // namespace
}  // namespace qv2x

extern "C" int qv2x_cam_heads_i8(const qv2x_cam_heads_desc* d, const int8_t* in, const int8_t* w_frag, const float* scale, const int32_t* corr,
                                 const int32_t* aw, const float* bias, float* depth, float* feats, void* stream) {
    using namespace qv2x;
    if (!d || !in || !w_frag || !scale || !corr || !aw || !bias || !depth || !feats) return fail(QV2X_EINVAL, "qv2x_cam_heads_i8: null pointer");
    if (d->views <= 0 || d->h <= 0 || d->w <= 0) return fail(QV2X_EINVAL, "qv2x_cam_heads_i8: views %d, h %d, w %d must be positive", d->views, d->h, d->w);
    if ((long long)d->views * d->h * d->w > 2147483647LL - 256) return fail(QV2X_EINVAL, "qv2x_cam_heads_i8: views * h * w is outside int32");
    if (d->depth_bins < 1 || d->depth_bins > 256) return fail(QV2X_EINVAL, "qv2x_cam_heads_i8: depth_bins %d outside 1..256", d->depth_bins);
    if (d->features < 4 || d->features > 256) return fail(QV2X_EINVAL, "qv2x_cam_heads_i8: features %d outside 4..256", d->features);
    if (d->features % 4) return fail(QV2X_EALIGN, "qv2x_cam_heads_i8: features %d %% 4 != 0", d->features);
    if (d->cin < 32 || d->cin > 4096 || d->cin % 32) return fail(QV2X_EALIGN, "qv2x_cam_heads_i8: cin %d must be a multiple of 32 in 32..4096", d->cin);
    if (!(d->depth_delta > 0.0f) || !(d->feat_delta > 0.0f)) return fail(QV2X_EINVAL, "qv2x_cam_heads_i8: depth_delta and feat_delta must be positive");
    if (!(d->depth_zp >= 0.0f && d->depth_zp <= 255.0f) || !(d->feat_zp >= 0.0f && d->feat_zp <= 255.0f))
        return fail(QV2X_EINVAL, "qv2x_cam_heads_i8: zero points in 0..255");
    if (((uintptr_t)in & 15) || ((uintptr_t)w_frag & 15) || ((uintptr_t)scale & 15) || ((uintptr_t)corr & 15) || ((uintptr_t)aw & 15) ||
        ((uintptr_t)bias & 15) || ((uintptr_t)depth & 3) || ((uintptr_t)feats & 3))
        return fail(QV2X_EALIGN, "qv2x_cam_heads_i8: in / w_frag / scale / corr / aw / bias 16-byte, depth / feats 4-byte aligned");
    HeadsArgs a;
    a.in = in; a.w = w_frag; a.scale = scale; a.corr = corr; a.aw = aw; a.bias = bias; a.depth = depth; a.feats = feats;
    a.views = d->views; a.h = d->h; a.wd = d->w; a.cin = d->cin; a.ks = d->cin / 32; a.D = d->depth_bins; a.C = d->features;
    a.dp = (d->depth_bins + 31) / 32 * 32;
    a.tiles_r = (a.dp + (d->features + 31) / 32 * 32) / 32;
    a.M = d->views * d->h * d->w;
    a.d_delta = d->depth_delta; a.d_rdelta = 1.0f / d->depth_delta; a.d_zp = d->depth_zp;
    a.f_delta = d->feat_delta; a.f_rdelta = 1.0f / d->feat_delta; a.f_zp = d->feat_zp;
    const int tiles = (a.M + 31) / 32;
    cam_heads_kernel<<<dim3((tiles + 3) / 4), 256, 0, (hipStream_t)stream>>>(a);
    return hip_check(hipGetLastError(), "qv2x_cam_heads_i8 launch");
}
