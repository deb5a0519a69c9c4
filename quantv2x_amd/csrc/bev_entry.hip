// Camera agents, the input side of the first QuantBasicBlock of a ResNetBEVBackbone on the lift-splat's fp32 BEV (quant_block.py:68-97 over
// base_bev_backbone_resnet.py): conv1 (3x3, stride 1 | 2, pad 1) -> ReLU -> activation quantizer -> codes, and the block's shortcut (the
// strided 1x1 `downsample`, or the pixel's own channels) as fp32 rows -- one launch, both outputs from one staging of the input.
//
// The map is NCHW and on no quantizer grid, so the sum is an fp32 chain; the contract (include/qv2x.h) orders it k = (ky*3 + kx)*cin + ci
// ascending from +0, which is what v_mfma_f32_32x32x2_f32 computes when K is walked in that order (deconv_f32.hip; tools/probes/mfma_probe.hip).
// GEMM view: columns = 32 output pixels of one output row, rows = 32 output channels, K = 9 cin.  As in deconv_f32.hip the WEIGHTS are the
// A operand: a lane ends with one pixel and sixteen channels in four runs of four, which requantize four at a time and leave as one 16-byte
// store after two v_permlane32_swap.
//
// A workgroup (two waves = the two 32-channel halves of 64 output channels) owns 32 consecutive pixels of one output row.  The chain order
// puts a tap's whole cin before the next tap, so for each ky the workgroup stages the ONE input row the tap row reads -- all cin channels,
// 31 s + 3 columns, zeros outside the map (fmaf(0, w, acc) = acc: the bits of skipping the tap) -- as [cin][columns] in LDS: this is the
// im2col, a B operand is then one ds_read_b32 at [ci][s * pixel + kx].  33 KB at cin 128, stride 2: four workgroups per CU, whose staging
// and MFMA phases overlap each other.  The weights [9 cin / 8][cout][2][4] come from L2 as one 16-byte load per four MFMAs, two groups ahead.
// The centre tap (ky = kx = 1) is the 1x1 shortcut's pixel: its B operands feed a second accumulator with the downsample weights.
#include "common.h"

#include <type_traits>

namespace qv2x {
namespace {

struct BevEntryArgs {
    const float* in; const float* w1; const float* b1; const float* wd; const float* bd; int8_t* out; float* sc;
    int n, h, w, cin, cout, s, ho, wo, ds, ncols;
    float out_delta, out_zp;
};

__global__ __launch_bounds__(128) void bev_entry_kernel(const BevEntryArgs a) {
    extern __shared__ __attribute__((aligned(16))) float row[];           // [cin][ncols]: the input row of the current ky
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, par = lane >> 5;
    const int cogs = a.cout >> 6;
    const int img = blockIdx.z / cogs, cog = blockIdx.z - img * cogs;
    const int yo = blockIdx.y, x0 = blockIdx.x * 32;
    const int co0 = cog * 64 + wave * 32;
    const int P = a.ncols;
    const int G = a.cin >> 3;                                               // groups of 8 k per tap
    const int total = 9 * G;

    // weights: [k / 8][cout][par][4], element j of the lane's float4 is k = 8 g + 2 j + par: MFMA k-step j of the group
    const float* w1p = a.w1 + ((size_t)(co0 + l31) * 2 + par) * 4;
    const float* wdp = a.wd + ((size_t)(co0 + l31) * 2 + par) * 4;
    const size_t gstride = (size_t)a.cout * 8;
    v4f ring[2];
    ring[0] = *(const v4f*)w1p;
    ring[1] = *(const v4f*)(w1p + gstride);                                 // (total >= 18)
    int g = 0;                                                              // the group ring[0] holds

    v16f acc, accs;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[r] = 0.0f; accs[r] = 0.0f; }

    const float* plane = a.in + (size_t)img * a.cin * a.h * a.w;
    const size_t cstride = (size_t)a.h * a.w;
    const int ix0 = x0 * a.s - 1;
    const float* xp = row + par * P + l31 * a.s;                            // + (8 gg + 2 j) * P + kx

    auto tap = [&](const int kx, auto with_shortcut) __attribute__((always_inline)) {
        constexpr bool SC = decltype(with_shortcut)::value;
        const float* xk = xp + kx;
        v4f sring[2];
        if constexpr (SC) { sring[0] = *(const v4f*)wdp; sring[1] = *(const v4f*)(wdp + gstride); }
        for (int gg = 0; gg < G; gg += 2) {                                 // (cin % 16 == 0: G is even)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const v4f wc = ring[u];
                const int nxt = g + 2 < total ? g + 2 : total - 1;         // (the last two re-read the last group)
                ring[u] = *(const v4f*)(w1p + (size_t)nxt * gstride);
                v4f ws;
                if constexpr (SC) {
                    ws = sring[u];
                    const int sn = gg + u + 2 < G ? gg + u + 2 : G - 1;
                    sring[u] = *(const v4f*)(wdp + (size_t)sn * gstride);
                }
                float x[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] = xk[(8 * (gg + u) + 2 * j) * P];
                __builtin_amdgcn_sched_barrier(0);                          // (the look-ahead loads stay in front of the MFMAs)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[j], x[j], acc, 0, 0, 0);
                    if constexpr (SC) accs = __builtin_amdgcn_mfma_f32_32x32x2f32(ws[j], x[j], accs, 0, 0, 0);
                }
                ++g;
            }
        }
    };

    const int ci_first = (int)threadIdx.x / P, c_first = (int)threadIdx.x - ci_first * P, ci_step = 128 / P, c_step = 128 - ci_step * P;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = yo * a.s + ky - 1;
        const bool yin = iy >= 0 && iy < a.h;
        if (ky) __syncthreads();                                            // every wave is done with the previous row
        const float* src = plane + (size_t)(yin ? iy : 0) * a.w;
        const int cnt = a.cin * P;
        int ci = ci_first, c = c_first;                                     // (channel, column) of element i, stepped without a divide
#pragma unroll 4
        for (int i = threadIdx.x; i < cnt; i += 128) {
            const int ix = ix0 + c;
            float v = 0.0f;
            if (yin && ix >= 0 && ix < a.w) v = src[(size_t)ci * cstride + ix];
            row[i] = v;
            ci += ci_step; c += c_step;
            if (c >= P) { c -= P; ++ci; }
        }
        __syncthreads();
        if (ky == 1 && !a.ds) {
            // identity shortcut (stride 1, cin == cout): the centre pixels' own channels, this workgroup's 64 of them
            for (int i = threadIdx.x; i < 32 * 16; i += 128) {
                const int p = i >> 4, ch = cog * 64 + 4 * (i & 15);
                if (x0 + p < a.wo) {
                    v4f v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = row[(ch + e) * P + p + 1];
                    *(v4f*)(a.sc + ((size_t)(img * a.ho + yo) * a.wo + x0 + p) * a.cout + ch) = v;
                }
            }
        }
        tap(0, std::false_type{});
        if (ky == 1 && a.ds) tap(1, std::true_type{});
        else tap(1, std::false_type{});
        tap(2, std::false_type{});
    }

    // lane: pixel x0 + l31, channels co0 + 8 q + 4 par + e (q = r >> 2, e = r & 3)
    const int xo = x0 + l31;
    const bool live = xo < a.wo;
    const float rd = 1.0f / a.out_delta, lowc = a.out_zp + 8388608.0f;      // the ReLU lives in the clamp (q_pack4)
    int pk[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const v4f b4 = *(const v4f*)(a.b1 + co0 + 8 * q + 4 * par);
        float yv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) yv[e] = acc[4 * q + e] + b4[e];
        pk[q] = q_pack4(yv[0], yv[1], yv[2], yv[3], a.out_delta, rd, a.out_zp, lowc);
    }
    // v_permlane32_swap turns the four quads (0-3 | 8-11 | 16-19 | 24-27 in the lower half-wave, +4 in the upper) into 16 consecutive channels
    const auto s02 = __builtin_amdgcn_permlane32_swap(pk[0], pk[2], false, false);
    const auto s13 = __builtin_amdgcn_permlane32_swap(pk[1], pk[3], false, false);
    v4i ob;
    ob[0] = s02[0]; ob[1] = s02[1]; ob[2] = s13[0]; ob[3] = s13[1];
    if (live)
        *(v4i*)(a.out + ((size_t)(img * (a.ho + 2) + yo + 1) * (a.wo + 2) + xo + 1) * a.cout + co0 + par * 16) = ob;
    if (a.ds && live) {
        float* dst = a.sc + ((size_t)(img * a.ho + yo) * a.wo + xo) * a.cout + co0 + 4 * par;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const v4f b4 = *(const v4f*)(a.bd + co0 + 8 * q + 4 * par);
            v4f y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = accs[4 * q + e] + b4[e];
            *(v4f*)(dst + 8 * q) = y;
        }
    }
}

}  // namespace
}  // namespace qv2x

extern "C" int qv2x_bev_entry_f32(const qv2x_bev_entry_desc* d, const float* in, const float* w1, const float* b1, const float* wd,
                                  const float* bd, int8_t* out, float* shortcut, void* stream) {
    using namespace qv2x;
    const char* who = "qv2x_bev_entry_f32";
    if (!d || !in || !w1 || !b1 || !out || !shortcut) return fail(QV2X_EINVAL, "%s: null pointer", who);
    if (d->downsample != 0 && d->downsample != 1) return fail(QV2X_EINVAL, "%s: downsample %d must be 0 or 1", who, d->downsample);
    if (d->downsample && (!wd || !bd)) return fail(QV2X_EINVAL, "%s: null pointer (the downsample's weights / bias)", who);
    if (d->n <= 0 || d->h <= 0 || d->w <= 0) return fail(QV2X_EINVAL, "%s: n %d, h %d, w %d must be positive", who, d->n, d->h, d->w);
    if (d->stride != 1 && d->stride != 2) return fail(QV2X_EINVAL, "%s: stride %d must be 1 or 2", who, d->stride);
    if (d->cin < 16 || d->cout < 64) return fail(QV2X_EINVAL, "%s: cin %d must be >= 16, cout %d >= 64", who, d->cin, d->cout);
    if (!(d->out_delta > 0.0f)) return fail(QV2X_EINVAL, "%s: out_delta must be positive", who);
    if (!(d->out_zp >= 0.0f && d->out_zp <= 255.0f)) return fail(QV2X_EINVAL, "%s: out_zp must be in 0..255", who);
    if (d->cin % 16 || d->cout % 64) return fail(QV2X_EALIGN, "%s: cin %% 16, cout %% 64", who);
    if (!d->downsample && (d->stride != 1 || d->cin != d->cout))
        return fail(QV2X_EINVAL, "%s: the identity shortcut needs stride 1 and cin == cout (stride %d, cin %d, cout %d)", who, d->stride, d->cin, d->cout);
    const int ho = (d->h - 1) / d->stride + 1, wo = (d->w - 1) / d->stride + 1, ncols = 31 * d->stride + 3;
    const long long lds = 4LL * d->cin * ncols;
    if (lds > 65536) return fail(QV2X_EINVAL, "%s: cin %d at stride %d needs %lld bytes of LDS for one input row (limit 65536)", who, d->cin, d->stride, lds);
    if (ho > 65535 || (long long)d->n * (d->cout / 64) > 65535 || (long long)d->n * (ho + 2) * (wo + 2) > 2147483647LL / d->cout
        || (long long)d->n * d->cin * d->h * d->w > 2147483647LL)
        return fail(QV2X_EINVAL, "%s: n %d x %d x %d x cin %d is outside the launch grid / int32", who, d->n, d->h, d->w, d->cin);
    if (((uintptr_t)in & 15) || ((uintptr_t)w1 & 15) || ((uintptr_t)b1 & 15) || ((uintptr_t)wd & 15) || ((uintptr_t)bd & 15)
        || ((uintptr_t)out & 15) || ((uintptr_t)shortcut & 15))
        return fail(QV2X_EALIGN, "%s: in, w1, b1, wd, bd, out, shortcut must be 16-byte aligned", who);
    BevEntryArgs a;
    a.in = in; a.w1 = w1; a.b1 = b1; a.wd = d->downsample ? wd : w1; a.bd = d->downsample ? bd : b1; a.out = out; a.sc = shortcut;
    a.n = d->n; a.h = d->h; a.w = d->w; a.cin = d->cin; a.cout = d->cout; a.s = d->stride; a.ho = ho; a.wo = wo; a.ds = d->downsample;
    a.ncols = ncols; a.out_delta = d->out_delta; a.out_zp = d->out_zp;
    const dim3 grid((unsigned)((wo + 31) / 32), (unsigned)ho, (unsigned)(d->n * (d->cout / 64)));
    bev_entry_kernel<<<grid, 128, (size_t)lds, (hipStream_t)stream>>>(a);
    return hip_check(hipGetLastError(), "qv2x_bev_entry_f32 launch");
}
