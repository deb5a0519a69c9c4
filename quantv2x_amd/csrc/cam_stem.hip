// Camera encoder, front end: conv1 (7x7, stride 2, pad 3, 3 -> 64, BN folded) of QuantCamEncode_Resnet101's trunk on the fp32 image, ReLU,
// the activation quantizer and the 3x3 stride-2 max-pool, one launch (opencood/quant/quant_block.py:744-860 over torchvision's ResNet stem).
//
// The contract (include/qv2x.h) pins the sum as an ascending (ky, kx, ci) fmaf chain from +0, so the kernel runs on VALU FMAs: one lane =
// one conv pixel x 16 output channels, the pixel's 147 taps read from an LDS patch of the image (zeros outside the image: fmaf(0, w, acc)
// = acc), the 16 weights of a tap wave-uniform and therefore fetched by scalar loads -- a v_fma per output per tap and nothing else in the
// loop.  2 * 147 * 64 flop per conv pixel is 1.85 GFMA for four 384 x 512 views: tens of microseconds on the f32 VALU, and the f32 MFMA
// (K padded to 148) would halve that at the price of a 4 x 4 im2col shuffle per tap; DESIGN.md section 14 has the arithmetic.
//
// A workgroup owns PT x PT pooled pixels: it computes the (2 PT + 1)^2 conv pixels under them (one ring of recomputation per tile, 13 %),
// keeps their codes in LDS and pools there, so the conv map never goes to memory.  A conv pixel outside Hc x Wc gets code 0, the lowest code
// there is: the pool's -inf padding (a window always holds its own centre, which is inside).
#include "common.h"

namespace qv2x {
namespace {

constexpr int PT = 8;                          // pooled tile
constexpr int CT = 2 * PT + 1;                 // conv tile: rows 2 P0 - 1 .. 2 P0 + 2 PT - 1
constexpr int NPIX = CT * CT;                  // 289
constexpr int NCHUNK = (NPIX + 63) / 64;       // wave-sized pieces of the conv tile
constexpr int IT = 2 * (CT - 1) + 7;           // image patch: rows 4 P0 - 5 .. 4 P0 + 4 PT + 1
constexpr int IP = IT + 1;                     // patch pitch in floats

struct StemArgs {
    const float* img; const float* w; const float* bias; int8_t* out;
    int views, h, wd, hc, wc, hp, wp;
    long long view_stride;
    float rdelta, zp;
};

__device__ __forceinline__ unsigned max_u8x4(unsigned a, unsigned b) {
    unsigned r = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned x = (a >> (8 * e)) & 255u, y = (b >> (8 * e)) & 255u;
        r |= (x > y ? x : y) << (8 * e);
    }
    return r;
}

__global__ __launch_bounds__(256) void cam_stem_kernel(const StemArgs a) {
    __shared__ float patch[3 * IT * IP];                                  // 18.7 KB
    __shared__ __attribute__((aligned(16))) unsigned codes[NCHUNK * 64 * 16];      // [conv pixel][64 code bytes], 20 KB
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int v = blockIdx.z, p0 = blockIdx.y * PT, q0 = blockIdx.x * PT;
    const int cr0 = 2 * p0 - 1, cc0 = 2 * q0 - 1;                         // first conv row / column of the tile
    const int ir0 = 2 * cr0 - 3, ic0 = 2 * cc0 - 3;                       // first image row / column of the patch
    const float* src = a.img + (size_t)v * (size_t)a.view_stride;
    for (int i = threadIdx.x; i < 3 * IT * IT; i += 256) {
        const int ci = i / (IT * IT), rem = i - ci * (IT * IT), py = rem / IT, px = rem - py * IT;
        const int iy = ir0 + py, ix = ic0 + px;
        float x = 0.0f;
        if (iy >= 0 && iy < a.h && ix >= 0 && ix < a.wd) x = src[((size_t)ci * a.h + iy) * a.wd + ix];
        patch[(ci * IT + py) * IP + px] = x;
    }
    __syncthreads();
    // wave tasks: (64-pixel chunk, 16-channel group); the group is wave-uniform, so the weights come through scalar loads
    for (int task = wave; task < NCHUNK * 4; task += 4) {
        const int chunk = task >> 2, cg = __builtin_amdgcn_readfirstlane(task & 3);
        const int pix = chunk * 64 + lane;
        const int r = pix / CT, c = pix - r * CT;
        const bool inside = pix < NPIX && cr0 + r >= 0 && cr0 + r < a.hc && cc0 + c >= 0 && cc0 + c < a.wc;
        const float* xp = patch + (pix < NPIX ? (2 * r) * IP + 2 * c : 0);
        const float* wp = a.w + 16 * cg;
        float acc[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        for (int ky = 0; ky < 7; ++ky)
            for (int kx = 0; kx < 7; ++kx)
#pragma unroll
                for (int ci = 0; ci < 3; ++ci) {
                    const float x = xp[(ci * IT + ky) * IP + kx];
                    const float* wt = wp + ((ky * 7 + kx) * 3 + ci) * 64;
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[e] = __builtin_fmaf(x, wt[e], acc[e]);
                }
        v4i packed;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            unsigned cw = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float y = fmaxf(acc[4 * g + e] + a.bias[16 * cg + 4 * g + e], 0.0f);
                cw = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fmaf(y, a.rdelta, a.zp), e, cw);     // rint, saturate to 0..255, byte e
            }
            packed[g] = inside ? (int)cw : 0;
        }
        *(v4i*)(codes + (size_t)pix * 16 + 4 * cg) = packed;
    }
    __syncthreads();
    // pool: one thread = one pooled pixel x 16 channels
    const int pl = threadIdx.x >> 2, piece = threadIdx.x & 3;
    const int pr = pl / PT, pc = pl - pr * PT;
    const int p = p0 + pr, q = q0 + pc;
    if (p >= a.hp || q >= a.wp) return;
    unsigned m[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const v4i cv = *(const v4i*)(codes + (size_t)((2 * pr + dy) * CT + 2 * pc + dx) * 16 + 4 * piece);
#pragma unroll
            for (int g = 0; g < 4; ++g) m[g] = max_u8x4(m[g], (unsigned)cv[g]);
        }
    v4i o;
#pragma unroll
    for (int g = 0; g < 4; ++g) o[g] = (int)(m[g] ^ 0x80808080u);
    *(v4i*)(a.out + (((size_t)v * (a.hp + 2) + p + 1) * (a.wp + 2) + q + 1) * 64 + 16 * piece) = o;
}

}  // namespace
}  // namespace qv2x

extern "C" int qv2x_cam_stem_f32(const qv2x_cam_stem_desc* d, const float* img, const float* wdeq, const float* bias, int8_t* out, void* stream) {
    using namespace qv2x;
    if (!d || !img || !wdeq || !bias || !out) return fail(QV2X_EINVAL, "qv2x_cam_stem_f32: null pointer");
    if (d->views <= 0 || d->h <= 0 || d->w <= 0) return fail(QV2X_EINVAL, "qv2x_cam_stem_f32: views %d, h %d, w %d must be positive", d->views, d->h, d->w);
    const long long hc = (d->h - 1) / 2 + 1, wc = (d->w - 1) / 2 + 1, hp = (hc - 1) / 2 + 1, wp = (wc - 1) / 2 + 1;
    if ((long long)d->views * hc * wc > 2147483647LL || d->views > 65535 || (hp + PT - 1) / PT > 65535)
        return fail(QV2X_EINVAL, "qv2x_cam_stem_f32: views %d x conv map %lld x %lld is outside int32 / the launch grid", d->views, hc, wc);
    if (d->view_stride < 3LL * d->h * d->w) return fail(QV2X_EINVAL, "qv2x_cam_stem_f32: view_stride %lld < 3 * h * w = %lld", (long long)d->view_stride, 3LL * d->h * d->w);
    if (!(d->out_delta > 0.0f) || !(d->out_zp >= 0.0f && d->out_zp <= 255.0f)) return fail(QV2X_EINVAL, "qv2x_cam_stem_f32: out_delta must be positive, out_zp in 0..255");
    if (((uintptr_t)img & 3) || ((uintptr_t)wdeq & 15) || ((uintptr_t)bias & 15) || ((uintptr_t)out & 15))
        return fail(QV2X_EALIGN, "qv2x_cam_stem_f32: img 4-byte, wdeq / bias / out 16-byte aligned");
    StemArgs a;
    a.img = img; a.w = wdeq; a.bias = bias; a.out = out;
    a.views = d->views; a.h = d->h; a.wd = d->w; a.hc = (int)hc; a.wc = (int)wc; a.hp = (int)hp; a.wp = (int)wp;
    a.view_stride = d->view_stride; a.rdelta = 1.0f / d->out_delta; a.zp = d->out_zp;
    dim3 grid((unsigned)((wp + PT - 1) / PT), (unsigned)((hp + PT - 1) / PT), (unsigned)d->views);
    cam_stem_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(a);
    return hip_check(hipGetLastError(), "qv2x_cam_stem_f32 launch");
}
