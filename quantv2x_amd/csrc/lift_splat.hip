// Lift-splat BEV pooling of the camera branch (get_geometry + voxel_pooling of the reference's LiftSplatShoot,
// opencood/models/lift_splat_shoot.py:89-181) as a plan and a splat; include/qv2x.h has the contract, quantv2x_amd/lift_splat.py the
// float64 statements the two are tested against.
//   PLAN (once per camera rig)
//   lss_views_kernel     one thread per view: inverse of post_rots and rots * inverse(intrins) in fp64 (closed form: adjugate / determinant)
//   lss_cells_kernel     one thread per frustum point: the geometry chain in fp64 from the f32 inputs, rounded once, then the reference's own
//                        f32 cell expression (truncation toward zero: a coordinate up to one cell below the range lands in cell 0);
//                        key = sample * cells + cell, or the value `total` for a dropped point (sorts behind every kept one)
//   hipCUB radix sort    pairs (key, flat point index): stable, so a cell's points stay in ascending point index
//   lss_heads_kernel     one thread per sorted position: the per-cell interval table [begin, end), the feature row of every sorted point,
//                        the kept count
//   SPLAT (every frame)
//   lss_softmax_kernel   one thread per (view, pixel): probabilities over the D bins.  The maximum is subtracted and the exponentials,
//                        their sum and the quotient are fp64, rounded to f32 once: a probability carries ONE f32 rounding whatever the
//                        logits' spread (an f32 `x - max` alone would cost |x - max| * 2^-24 relative).  589 824 exponentials per OPV2V
//                        agent: noise next to the splat.  mode 'probs' skips it and reads the caller's tensor.
//   lss_transpose_kernel feats [view][C][pixel] -> [view][pixel][C]: the splat reads all channels of ONE pixel per point, contiguous
//                        here (C * 4 bytes: 16 B per lane), 4-byte gathers C cache lines apart in the caller's layout.
//   lss_splat_kernel     one workgroup per tile of TX consecutive cells of one BEV row, all C channels.  C / 4 threads own a cell (a float4
//                        of channels each) and walk ITS WHOLE interval in plan order: acc += p * f, one rounded product and one rounded
//                        add per point and channel, in fp32, no atomics.  Nothing is chunked, so an interval of any length (one cell of
//                        4 608 points next to cells of one) keeps its order; what a long interval costs is latency: eight points' loads
//                        are issued before their adds, with the next eight list entries already on their way.  The longest cell's
//                        chain bounds the kernel (DESIGN.md section 13 has the measurement).  The tile then goes through LDS so that
//                        every channel's TX cells leave as one contiguous run: each element of `out` is written exactly once, empty
//                        cells as +0.
// The order of every sum is a function of the plan alone: the same inputs give the same bits on every call, eager or replayed.
// The library is built with -ffp-contract=off: no multiply-add below is fused, in the fp64 chain or in the accumulation.
#include <hipcub/hipcub.hpp>

#include <math.h>

#include "common.h"

namespace qv2x {

namespace {

constexpr int LSS_MAX_VIEWS = 64, LSS_MAX_D = 128, LSS_MAX_C = 256;
constexpr int LSS_THREADS = 256;
constexpr int LSS_TILE_FLOATS = 4096;           // C * TX of the splat's LDS tile (16 KiB + padding): at C = 128 a tile is 32 cells, a 128-byte run per channel
constexpr int LSS_BATCH = 8;                    // points whose loads a thread keeps in flight together
constexpr int LSS_TP = 32;                      // pixels per workgroup of the transpose
constexpr int LSS_MAGIC = 0x4c535331;           // "LSS1": the plan's signature in the workspace header

struct LssView { double pinv[9], m[9], pt[3], tr[3]; };        // inverse(post_rots), rots * inverse(intrins), post_trans, trans

struct LssHeader { int magic, points, total, kept; };

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

struct LssLayout {
    long long P, total, ncell, dhw, fhw;
    int views, end_bit;
    size_t header, viewmats, pts, iv, keys_in, keys_out, vals_in, vals_out, probs, feat_t, cub, cub_bytes, bytes;
};

int bit_width(unsigned long long v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }

// `sort`: size the plan's sort scratch too (a hipCUB query on the host).  It is the LAST region, so the splat, which never sorts and runs
// every frame, leaves the query out and finds every other region at the same offset.
int lss_check(const qv2x_lss_desc* d, const char* who, LssLayout* L, bool sort = true) {
    if (!d) return fail(QV2X_EINVAL, "%s: null descriptor", who);
    if (d->samples < 1 || d->views < 1 || (long long)d->samples * d->views > LSS_MAX_VIEWS)
        return fail(QV2X_EINVAL, "%s: samples %d x views %d: 1..%d views in all", who, d->samples, d->views, LSS_MAX_VIEWS);
    if (d->depth_bins < 1 || d->depth_bins > LSS_MAX_D) return fail(QV2X_EINVAL, "%s: depth_bins %d: 1..%d", who, d->depth_bins, LSS_MAX_D);
    if (d->fh < 1 || d->fw < 1) return fail(QV2X_EINVAL, "%s: feature map %d x %d: both >= 1", who, d->fh, d->fw);
    if (d->features < 8 || d->features > LSS_MAX_C || d->features % 8)
        return fail(QV2X_EINVAL, "%s: features %d: a multiple of 8 in 8..%d", who, d->features, LSS_MAX_C);
    for (int i = 0; i < 3; ++i) {
        if (d->nx[i] < 1) return fail(QV2X_EINVAL, "%s: nx[%d] = %d: >= 1", who, i, d->nx[i]);
        if (!(d->dx[i] > 0.0f) || !isfinite(d->dx[i]) || !isfinite(d->bx[i]))
            return fail(QV2X_EINVAL, "%s: dx[%d] = %g, bx[%d] = %g: dx > 0, both finite", who, i, (double)d->dx[i], i, (double)d->bx[i]);
    }
    const long long views = (long long)d->samples * d->views;
    const double cells = (double)d->samples * d->nx[0] * d->nx[1] * d->nx[2];
    if (cells > 2147483647.0) return fail(QV2X_EINVAL, "%s: samples x nx[0] x nx[1] x nx[2] = %.0f cells exceed int32", who, cells);
    const double points = (double)views * d->depth_bins * d->fh * d->fw;
    if (points > 2147483647.0) return fail(QV2X_EINVAL, "%s: %.0f frustum points exceed int32", who, points);
    if ((double)views * d->fh * d->fw * d->features > 2147483647.0)
        return fail(QV2X_EINVAL, "%s: views x fh x fw x features = %.0f exceeds int32", who, (double)views * d->fh * d->fw * d->features);
    if (L) {
        L->views = (int)views;
        L->fhw = (long long)d->fh * d->fw;
        L->dhw = L->fhw * d->depth_bins;
        L->P = views * L->dhw;
        L->ncell = (long long)d->nx[0] * d->nx[1] * d->nx[2];
        L->total = L->ncell * d->samples;
        L->end_bit = bit_width((unsigned long long)L->total);           // the field holds the VALUE total too: the dropped points' key
        size_t o = 0;
        auto take = [&o](size_t bytes) { const size_t at = o; o += align_up(bytes); return at; };
        L->header = take(sizeof(LssHeader));
        L->viewmats = take(sizeof(LssView) * LSS_MAX_VIEWS);
        L->pts = take((size_t)L->P * 8);
        L->iv = take((size_t)L->total * 8);
        L->keys_in = take((size_t)L->P * 4);
        L->keys_out = take((size_t)L->P * 4);
        L->vals_in = take((size_t)L->P * 4);
        L->vals_out = take((size_t)L->P * 4);
        L->probs = take((size_t)L->P * 4);
        L->feat_t = take((size_t)views * L->fhw * d->features * 4);
        L->cub_bytes = 0;
        if (sort) {
            // the size query launches nothing.  Its status is dropped on purpose (as in csrc/voxelize.hip): on a host without a device it
            // reports the missing device, and qv2x_lss_workspace_bytes has to answer there too (the limits are tested without a GPU).
            (void)hipcub::DeviceRadixSort::SortPairs(nullptr, L->cub_bytes, (unsigned*)nullptr, (unsigned*)nullptr, (int*)nullptr, (int*)nullptr,
                                                     (int)L->P, 0, L->end_bit);
        }
        L->cub = take(L->cub_bytes);
        L->bytes = o;
    }
    return QV2X_OK;
}

// adjugate / determinant of a row-major 3x3 (quantv2x_amd/lift_splat.py: inv3_statement has the same lines)
__device__ void inv3(const double* a, double* o) {
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[2] * a[7] - a[1] * a[8], c02 = a[1] * a[5] - a[2] * a[4];
    const double c10 = a[5] * a[6] - a[3] * a[8], c11 = a[0] * a[8] - a[2] * a[6], c12 = a[2] * a[3] - a[0] * a[5];
    const double c20 = a[3] * a[7] - a[4] * a[6], c21 = a[1] * a[6] - a[0] * a[7], c22 = a[0] * a[4] - a[1] * a[3];
    const double det = (a[0] * c00 + a[1] * c10) + a[2] * c20;
    o[0] = c00 / det; o[1] = c01 / det; o[2] = c02 / det;
    o[3] = c10 / det; o[4] = c11 / det; o[5] = c12 / det;
    o[6] = c20 / det; o[7] = c21 / det; o[8] = c22 / det;
}

__global__ void lss_views_kernel(int views, const float* __restrict__ rots, const float* __restrict__ trans, const float* __restrict__ intrins,
                                 const float* __restrict__ post_rots, const float* __restrict__ post_trans, LssView* __restrict__ out) {
    const int v = (int)threadIdx.x;
    if (v >= views) return;
    double a[9], k[9], r[9];
    LssView o;
    for (int i = 0; i < 9; ++i) { a[i] = (double)post_rots[v * 9 + i]; r[i] = (double)rots[v * 9 + i]; }
    inv3(a, o.pinv);
    for (int i = 0; i < 9; ++i) a[i] = (double)intrins[v * 9 + i];
    inv3(a, k);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o.m[i * 3 + j] = (r[i * 3] * k[j] + r[i * 3 + 1] * k[3 + j]) + r[i * 3 + 2] * k[6 + j];
    for (int i = 0; i < 3; ++i) { o.pt[i] = (double)post_trans[v * 3 + i]; o.tr[i] = (double)trans[v * 3 + i]; }
    out[v] = o;
}

struct LssPlanArgs {
    int P, total, ncell, dhw, fhw, views_per_sample;
    int nx[3];
    float dx[3], lo[3];                         // lo = fl(bx - dx / 2): the reference's own lower bound
    const float* frustum; const LssView* views;
    unsigned* keys; int* vals; int* cells_out;
};

// one axis of `((g - (bx - dx/2)) / dx).long()` with the kept test 0 <= i < n: the index, or -1
__device__ __forceinline__ int lss_axis(float g, float lo, float dx, int n) {
    const float t = (g - lo) / dx;
    if (!(t > -1.0f && t < 2147483648.0f)) return -1;               // (a NaN fails both; trunc(t) >= 0 iff t > -1)
    const int i = (int)t;                                           // toward zero
    return i < n ? i : -1;
}

__global__ __launch_bounds__(LSS_THREADS) void lss_cells_kernel(const LssPlanArgs a) {
    const int p = (int)(blockIdx.x * (unsigned)LSS_THREADS + threadIdx.x);
    if (p >= a.P) return;
    const int view = p / a.dhw, r = p - view * a.dhw;
    const LssView& V = a.views[view];
    const float* f = a.frustum + (size_t)r * 3;
    const double q0 = (double)f[0] - V.pt[0], q1 = (double)f[1] - V.pt[1], q2 = (double)f[2] - V.pt[2];
    const double u0 = (V.pinv[0] * q0 + V.pinv[1] * q1) + V.pinv[2] * q2;
    const double u1 = (V.pinv[3] * q0 + V.pinv[4] * q1) + V.pinv[5] * q2;
    const double u2 = (V.pinv[6] * q0 + V.pinv[7] * q1) + V.pinv[8] * q2;
    const double w0 = u0 * u2, w1 = u1 * u2;
    const float gx = (float)(((V.m[0] * w0 + V.m[1] * w1) + V.m[2] * u2) + V.tr[0]);
    const float gy = (float)(((V.m[3] * w0 + V.m[4] * w1) + V.m[5] * u2) + V.tr[1]);
    const float gz = (float)(((V.m[6] * w0 + V.m[7] * w1) + V.m[8] * u2) + V.tr[2]);
    int cell = -1;
    if (isfinite(gx) && isfinite(gy) && isfinite(gz)) {
        const int ix = lss_axis(gx, a.lo[0], a.dx[0], a.nx[0]), iy = lss_axis(gy, a.lo[1], a.dx[1], a.nx[1]),
                  iz = lss_axis(gz, a.lo[2], a.dx[2], a.nx[2]);
        if ((ix | iy | iz) >= 0) cell = (iz * a.nx[1] + iy) * a.nx[0] + ix;
    }
    a.cells_out[p] = cell;
    a.keys[p] = cell >= 0 ? (unsigned)((view / a.views_per_sample) * a.ncell + cell) : (unsigned)a.total;
    a.vals[p] = p;
}

// (a kernel, not a memset node: csrc/voxelize.hip says why)
__global__ void lss_clear_kernel(int2* __restrict__ iv, int total, LssHeader* __restrict__ hdr, int P) {
    const int stride = (int)(gridDim.x * blockDim.x);
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += stride) iv[k] = make_int2(0, 0);
    if (blockIdx.x == 0 && threadIdx.x == 0) { hdr->magic = LSS_MAGIC; hdr->points = P; hdr->total = total; hdr->kept = 0; }
}

__global__ __launch_bounds__(LSS_THREADS) void lss_heads_kernel(const unsigned* __restrict__ keys, const int* __restrict__ vals, int P,
                                                                unsigned total, int dhw, int fhw, int2* __restrict__ pts,
                                                                int2* __restrict__ iv, LssHeader* __restrict__ hdr) {
    const int j = (int)(blockIdx.x * (unsigned)LSS_THREADS + threadIdx.x);
    if (j >= P) return;
    const unsigned k = keys[j];
    if (k >= total) return;
    const int p = vals[j], view = p / dhw;
    pts[j] = make_int2(p, view * fhw + (p - view * dhw) % fhw);     // (point, row of the transposed feature map)
    if (j == 0 || keys[j - 1] != k) iv[k].x = j;
    const unsigned next = j + 1 < P ? keys[j + 1] : total;
    if (next != k) iv[k].y = j + 1;
    if (next >= total) hdr->kept = j + 1;                           // the last kept position: one thread
}

// ---- splat ----------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(LSS_THREADS) void lss_softmax_kernel(const float* __restrict__ logits, int views, int D, int fhw,
                                                                  float* __restrict__ probs) {
    const int i = (int)(blockIdx.x * (unsigned)LSS_THREADS + threadIdx.x);
    if (i >= views * fhw) return;
    const int view = i / fhw, hw = i - view * fhw;
    const float* x = logits + (size_t)view * D * fhw + hw;
    float m = x[0];
    for (int d = 1; d < D; ++d) m = fmaxf(m, x[(size_t)d * fhw]);
    double s = 0.0;
    for (int d = 0; d < D; ++d) s += exp((double)x[(size_t)d * fhw] - (double)m);
    float* o = probs + (size_t)view * D * fhw + hw;
    for (int d = 0; d < D; ++d) o[(size_t)d * fhw] = (float)(exp((double)x[(size_t)d * fhw] - (double)m) / s);
}

// grid (pixel tiles of LSS_TP, views); dynamic LDS C * (LSS_TP + 1) floats
__global__ __launch_bounds__(LSS_THREADS) void lss_transpose_kernel(const float* __restrict__ feats, int C, int fhw, float* __restrict__ out) {
    extern __shared__ float tile[];
    const int tid = (int)threadIdx.x, view = (int)blockIdx.y, hw0 = (int)blockIdx.x * LSS_TP;
    const int n = fhw - hw0 < LSS_TP ? fhw - hw0 : LSS_TP;
    const float* src = feats + (size_t)view * C * fhw + hw0;
    for (int i = tid; i < C * LSS_TP; i += LSS_THREADS) {
        const int c = i / LSS_TP, hw = i % LSS_TP;
        if (hw < n) tile[c * (LSS_TP + 1) + hw] = src[(size_t)c * fhw + hw];
    }
    __syncthreads();
    float* dst = out + ((size_t)view * fhw + hw0) * C;
    for (int i = tid; i < C * n; i += LSS_THREADS) {
        const int hw = i / C, c = i - hw * C;
        dst[i] = tile[c * (LSS_TP + 1) + hw];
    }
}

struct LssSplatArgs {
    int C, TX, X, Y, Z, tiles_x, ncell, P, total;
    const LssHeader* hdr; const int2* pts; const int2* iv;
    const float* probs; const float4* feat_t;
    float* out;
};

__device__ __forceinline__ void lss_add(float4& acc, float p, const float4 f) {
    acc.x += p * f.x; acc.y += p * f.y; acc.z += p * f.z; acc.w += p * f.w;
}

// grid: samples * Z * Y * tiles_x; dynamic LDS C * (TX + 1) floats
__global__ __launch_bounds__(LSS_THREADS) void lss_splat_kernel(const LssSplatArgs a) {
    extern __shared__ float tile[];
    const int tid = (int)threadIdx.x, q = a.C >> 2, slots = LSS_THREADS / q, slot = tid / q, cq = tid - slot * q;
    const int tx = (int)(blockIdx.x % (unsigned)a.tiles_x), row = (int)(blockIdx.x / (unsigned)a.tiles_x);     // row = (b * Z + z) * Y + y
    const int zy_rows = a.Z * a.Y, b = row / zy_rows, zy = row - b * zy_rows, x0 = tx * a.TX;
    const int ncells = a.X - x0 < a.TX ? a.X - x0 : a.TX, ld = a.TX + 1;
    // a workspace no plan of THIS shape was written to holds no interval table: every cell reads as empty
    const bool planned = a.hdr->magic == LSS_MAGIC && a.hdr->points == a.P && a.hdr->total == a.total;
    const int kept = planned ? a.hdr->kept : 0;
    if (slot < slots) {
        const int2* iv = a.iv + (size_t)b * a.ncell + (size_t)zy * a.X + x0;
        for (int cx = slot; cx < ncells; cx += slots) {
            int2 r = planned ? iv[cx] : make_int2(0, 0);
            if (r.x < 0) r.x = 0;
            if (r.y > kept) r.y = kept;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r.y > r.x) {
                // batches of LSS_BATCH points: a batch's probabilities and feature rows are fetched together while the NEXT batch's list
                // entries are already on their way; the adds stay in plan order.  Past the interval's end the last entry is fetched again
                // (a valid address) and not added.
                const int last = r.y - 1;
                int2 cur[LSS_BATCH], nxt[LSS_BATCH];
#pragma unroll
                for (int u = 0; u < LSS_BATCH; ++u) cur[u] = a.pts[r.x + u < last ? r.x + u : last];
                for (int j = r.x; j < r.y; j += LSS_BATCH) {
                    float w[LSS_BATCH];
                    float4 f[LSS_BATCH];
#pragma unroll
                    for (int u = 0; u < LSS_BATCH; ++u) { w[u] = a.probs[cur[u].x]; f[u] = a.feat_t[(size_t)cur[u].y * q + cq]; }
#pragma unroll
                    for (int u = 0; u < LSS_BATCH; ++u) nxt[u] = a.pts[j + LSS_BATCH + u < last ? j + LSS_BATCH + u : last];
#pragma unroll
                    for (int u = 0; u < LSS_BATCH; ++u) if (j + u < r.y) lss_add(acc, w[u], f[u]);
#pragma unroll
                    for (int u = 0; u < LSS_BATCH; ++u) cur[u] = nxt[u];
                }
            }
            float* t = tile + (cq * 4) * ld + cx;
            t[0] = acc.x; t[ld] = acc.y; t[2 * ld] = acc.z; t[3 * ld] = acc.w;
        }
    }
    __syncthreads();
    const int z = zy / a.Y, y = zy - z * a.Y;
    const size_t plane = (size_t)a.Y * a.X;
    float* out = a.out + ((size_t)b * a.Z + z) * a.C * plane + (size_t)y * a.X + x0;
    for (int i = tid; i < a.C * a.TX; i += LSS_THREADS) {
        const int c = i / a.TX, x = i - c * a.TX;
        if (x < ncells) out[(size_t)c * plane + x] = tile[c * ld + x];
    }
}

}  // namespace

}  // namespace qv2x

extern "C" int64_t qv2x_lss_workspace_bytes(const qv2x_lss_desc* d) {
    using namespace qv2x;
    LssLayout L{};
    if (lss_check(d, "qv2x_lss_workspace_bytes", &L)) return -1;
    return (int64_t)L.bytes;
}

extern "C" int qv2x_lss_plan_f32(const qv2x_lss_desc* d, const float* frustum, const float* rots, const float* trans, const float* intrins,
                                 const float* post_rots, const float* post_trans, int32_t* cells_out, void* workspace, void* stream) {
    using namespace qv2x;
    const char* who = "qv2x_lss_plan_f32";
    LssLayout L{};
    if (int rc = lss_check(d, who, &L)) return rc;
    if (!frustum || !rots || !trans || !intrins || !post_rots || !post_trans || !cells_out || !workspace) return fail(QV2X_EINVAL, "%s: null pointer", who);
    if ((uintptr_t)workspace & 15) return fail(QV2X_EALIGN, "%s: workspace must be 16-byte aligned", who);
    char* w = (char*)workspace;
    hipStream_t st = (hipStream_t)stream;
    LssHeader* hdr = (LssHeader*)(w + L.header);
    LssView* views = (LssView*)(w + L.viewmats);
    LssPlanArgs a{};
    a.P = (int)L.P; a.total = (int)L.total; a.ncell = (int)L.ncell; a.dhw = (int)L.dhw; a.fhw = (int)L.fhw; a.views_per_sample = d->views;
    for (int i = 0; i < 3; ++i) { a.nx[i] = d->nx[i]; a.dx[i] = d->dx[i]; a.lo[i] = d->bx[i] - d->dx[i] / 2.0f; }
    a.frustum = frustum; a.views = views;
    a.keys = (unsigned*)(w + L.keys_in); a.vals = (int*)(w + L.vals_in); a.cells_out = cells_out;
    const unsigned G = (unsigned)((L.P + LSS_THREADS - 1) / LSS_THREADS);
    lss_clear_kernel<<<1024, LSS_THREADS, 0, st>>>((int2*)(w + L.iv), (int)L.total, hdr, (int)L.P);
    lss_views_kernel<<<1, LSS_MAX_VIEWS, 0, st>>>(L.views, rots, trans, intrins, post_rots, post_trans, views);
    lss_cells_kernel<<<G, LSS_THREADS, 0, st>>>(a);
    size_t tb = L.cub_bytes;
    if (int rc = hip_check(hipcub::DeviceRadixSort::SortPairs(w + L.cub, tb, a.keys, (unsigned*)(w + L.keys_out), a.vals, (int*)(w + L.vals_out),
                                                               (int)L.P, 0, L.end_bit, st), "lift-splat plan sort")) return rc;
    lss_heads_kernel<<<G, LSS_THREADS, 0, st>>>((const unsigned*)(w + L.keys_out), (const int*)(w + L.vals_out), (int)L.P, (unsigned)L.total,
                                                 (int)L.dhw, (int)L.fhw, (int2*)(w + L.pts), (int2*)(w + L.iv), hdr);
    return hip_check(hipGetLastError(), who);
}

extern "C" int qv2x_lss_splat_f32(const qv2x_lss_desc* d, const float* depth, const float* feats, int mode, void* workspace, float* out,
                                  void* stream) {
    using namespace qv2x;
    const char* who = "qv2x_lss_splat_f32";
    LssLayout L{};
    if (int rc = lss_check(d, who, &L, false)) return rc;
    if (mode != QV2X_LSS_LOGITS && mode != QV2X_LSS_PROBS) return fail(QV2X_EINVAL, "%s: mode %d: 0 (logits) or 1 (probabilities)", who, mode);
    if (!depth || !feats || !workspace || !out) return fail(QV2X_EINVAL, "%s: null pointer", who);
    if ((uintptr_t)workspace & 15) return fail(QV2X_EALIGN, "%s: workspace must be 16-byte aligned", who);
    char* w = (char*)workspace;                                      // (the splat's own scratch lives there: probabilities, transposed features)
    hipStream_t st = (hipStream_t)stream;
    const int C = d->features, fhw = (int)L.fhw;
    float* probs = (float*)(w + L.probs);
    float* feat_t = (float*)(w + L.feat_t);
    if (mode == QV2X_LSS_LOGITS)
        lss_softmax_kernel<<<(unsigned)((L.views * L.fhw + LSS_THREADS - 1) / LSS_THREADS), LSS_THREADS, 0, st>>>(depth, L.views, d->depth_bins, fhw, probs);
    lss_transpose_kernel<<<dim3((unsigned)((fhw + LSS_TP - 1) / LSS_TP), (unsigned)L.views), LSS_THREADS, (size_t)C * (LSS_TP + 1) * 4, st>>>(feats, C, fhw, feat_t);
    LssSplatArgs a{};
    a.C = C; a.TX = LSS_TILE_FLOATS / C < 64 ? LSS_TILE_FLOATS / C : 64;
    a.X = d->nx[0]; a.Y = d->nx[1]; a.Z = d->nx[2];
    a.tiles_x = (a.X + a.TX - 1) / a.TX; a.ncell = (int)L.ncell; a.P = (int)L.P; a.total = (int)L.total;
    const long long groups = (long long)d->samples * a.Z * a.Y * a.tiles_x;
    if (groups > 0x7fffffff) return fail(QV2X_EINVAL, "%s: %lld tiles exceed the grid", who, groups);
    a.hdr = (const LssHeader*)(w + L.header); a.pts = (const int2*)(w + L.pts); a.iv = (const int2*)(w + L.iv);
    a.probs = mode == QV2X_LSS_LOGITS ? probs : depth; a.feat_t = (const float4*)feat_t; a.out = out;
    lss_splat_kernel<<<(unsigned)groups, LSS_THREADS, (size_t)C * (a.TX + 1) * 4, st>>>(a);
    return hip_check(hipGetLastError(), who);
}
