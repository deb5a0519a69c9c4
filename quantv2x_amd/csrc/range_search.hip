// The MSE range search of the PTQ observers on the GPU: perform_2D_search / perform_1D_search of the reference
// (opencood/quant/quant_layer.py:201-254) score K (delta, zero point) candidates with one pass over the tensor and about thirty torch launches
// EACH; here the K pairs are a table built up front and every candidate is scored in one call (include/qv2x.h has the contract).
//   rs_partial_kernel  one workgroup of 256 threads per (channel, data slice, tile of 256 candidates).  A lane OWNS one candidate: delta,
//                      fl(1 / delta) and zp stay in registers.  The slice is staged through LDS in chunks of 1024 floats and read back as
//                      float4 with the same address in every lane -- a broadcast, no bank conflict -- so a lane sees the elements in
//                      element order and its fp64 sum needs no cross-lane step.  The work is VALU: per evaluation about 14 plain
//                      instructions, v_log_f32 + v_exp_f32 (quarter rate), one conversion and one fp64 add.
//   rs_reduce_kernel   one workgroup per channel: a thread adds the slices' partial sums of its candidates in slice order, divides by the
//                      element count, and keeps its first least loss; 256 (loss, k) pairs are then folded through LDS, lower k on a tie.
// Slices: per-channel weights (many short rows) give enough workgroups by themselves and take one slice; a per-tensor activation (one long
// row) is cut so that at most RS_TARGET_GROUPS workgroups exist.  The cut is a function of the descriptor alone -- not of the device -- so the
// summation order, and with it every bit of the result, is fixed by the shape.
// The library is built with -ffp-contract=off: the one fused operation below is written as fmaf.
#include "common.h"

namespace qv2x {

namespace {

constexpr int RS_THREADS = 256;             // candidates per tile
constexpr int RS_CHUNK = 1024;              // floats staged per round (4 KiB of LDS: eight workgroups fit a CU with room to spare)
constexpr int RS_MAX_SLICES = 128;
constexpr int64_t RS_TARGET_GROUPS = 1024;  // 256 CUs x 4 workgroups

struct RsShape { int64_t tiles, chunks, chunks_per_slice, slices, groups; };

RsShape rs_shape(const qv2x_range_search_desc* d) {
    RsShape s{};
    s.tiles = (d->candidates + RS_THREADS - 1) / RS_THREADS;
    s.chunks = (d->per_channel + RS_CHUNK - 1) / RS_CHUNK;
    const int64_t rows = (int64_t)d->channels * s.tiles;
    int64_t want = RS_TARGET_GROUPS / rows;                                   // rounded down: at most four workgroups on a CU, never a fifth on some
    if (want > RS_MAX_SLICES) want = RS_MAX_SLICES;
    if (want > s.chunks) want = s.chunks;
    if (want < 1) want = 1;
    s.chunks_per_slice = (s.chunks + want - 1) / want;
    s.slices = (s.chunks + s.chunks_per_slice - 1) / s.chunks_per_slice;      // every slice holds at least one element
    s.groups = rows * s.slices;
    return s;
}

int rs_check(const qv2x_range_search_desc* d, const char* who) {
    if (!d) return fail(QV2X_EINVAL, "%s: null descriptor", who);
    if (d->channels < 1) return fail(QV2X_EINVAL, "%s: channels >= 1", who);
    if (d->per_channel < 1) return fail(QV2X_EINVAL, "%s: per_channel >= 1", who);
    if (d->candidates < 1 || d->candidates > 65536) return fail(QV2X_EINVAL, "%s: candidates in 1..65536", who);
    if (d->n_levels < 4 || d->n_levels > 256) return fail(QV2X_EINVAL, "%s: n_levels in 4..256", who);
    if (d->per_channel > (int64_t)1 << 40 || (int64_t)d->channels * d->per_channel > (int64_t)1 << 40)
        return fail(QV2X_EINVAL, "%s: more than 2^40 elements", who);
    if (rs_shape(d).groups > 0x7fffffff) return fail(QV2X_EINVAL, "%s: channels x candidate tiles x slices exceeds the grid", who);
    return QV2X_OK;
}

struct RsArgs {
    int channels, candidates, tiles, slices;
    int64_t per_channel, slice_len;
    float top;                                  // n_levels - 1
    const float* x; const float* delta; const float* zp;
    double* partial;                            // [channels][slices][candidates]
    double* loss; int* best;
};

// |x - q|^2.4 of one element under one candidate
__device__ __forceinline__ float rs_term(float x, float delta, float rdelta, float zp, float top) {
    const float t = x * rdelta;
    float k = rintf(t);
    // t is within |x / delta| * 1.8e-7 of fl(x / delta): below 1100 that is < 2e-4, so both round to k unless t sits within 3e-4 of a
    // half-integer; at or above 1100 either value clamps (0 <= zp, top <= 255).  One lane in 1700 redoes the division.
    if ((fabsf(t - k) > 0.4997f) & (fabsf(t) < 1100.0f)) k = rintf(x / delta);
    const float code = fminf(fmaxf(k + zp, 0.0f), top);
    const float e = fabsf(__builtin_fmaf(zp - code, delta, x));         // zp - code is an exact integer: x - (code - zp) * delta, rounded once
    return e * e * __builtin_amdgcn_exp2f(0.4f * __builtin_amdgcn_logf(e));     // v_log_f32(0) = -inf, v_exp_f32(-inf) = 0
}

__global__ __launch_bounds__(RS_THREADS) void rs_partial_kernel(const RsArgs a) {
    __shared__ float4 stage4[RS_CHUNK / 4];
    float* stage = reinterpret_cast<float*>(stage4);
    const int tid = (int)threadIdx.x;
    const unsigned g = blockIdx.x;                                      // ((channel * slices) + slice) * tiles + tile
    const int tile = (int)(g % (unsigned)a.tiles);
    const unsigned cs = g / (unsigned)a.tiles;
    const int slice = (int)(cs % (unsigned)a.slices), c = (int)(cs / (unsigned)a.slices);
    const int k = tile * RS_THREADS + tid;
    const int kk = k < a.candidates ? k : a.candidates - 1;            // the lanes past the table score its last row and store nothing
    const float delta = a.delta[(int64_t)kk * a.channels + c], zp = a.zp[(int64_t)kk * a.channels + c];
    const float rdelta = 1.0f / delta, top = a.top;
    const float* row = a.x + (int64_t)c * a.per_channel;
    const int64_t begin = (int64_t)slice * a.slice_len;
    int64_t end = begin + a.slice_len;
    if (end > a.per_channel) end = a.per_channel;
    double acc = 0.0;
    for (int64_t base = begin; base < end; base += RS_CHUNK) {
        const int n = (int)(end - base < RS_CHUNK ? end - base : RS_CHUNK);
        __syncthreads();                                                // the previous chunk has been read by every wave
        float fetched[RS_CHUNK / RS_THREADS];
#pragma unroll
        for (int j = 0; j < RS_CHUNK / RS_THREADS; ++j) {               // the loads first, so that they are in flight together
            const int i = tid + j * RS_THREADS;
            fetched[j] = row[base + (i < n ? i : n - 1)];
        }
#pragma unroll
        for (int j = 0; j < RS_CHUNK / RS_THREADS; ++j) stage[tid + j * RS_THREADS] = fetched[j];
        __syncthreads();
        const int n4 = n & ~3;
        for (int i = 0; i < n4; i += 4) {
            const float4 v = stage4[i >> 2];                            // the same address in every lane: one broadcast read
            acc += (double)rs_term(v.x, delta, rdelta, zp, top);
            acc += (double)rs_term(v.y, delta, rdelta, zp, top);
            acc += (double)rs_term(v.z, delta, rdelta, zp, top);
            acc += (double)rs_term(v.w, delta, rdelta, zp, top);
        }
        for (int i = n4; i < n; ++i) acc += (double)rs_term(stage[i], delta, rdelta, zp, top);
    }
    if (k < a.candidates) a.partial[((int64_t)c * a.slices + slice) * a.candidates + k] = acc;
}

__device__ __forceinline__ bool rs_better(double l, int k, double bl, int bk) { return l < bl || (l == bl && k < bk); }

__global__ __launch_bounds__(RS_THREADS) void rs_reduce_kernel(const RsArgs a) {
    __shared__ double s_loss[RS_THREADS];
    __shared__ int s_k[RS_THREADS];
    const int tid = (int)threadIdx.x, c = (int)blockIdx.x;
    const double* part = a.partial + (int64_t)c * a.slices * a.candidates;
    const double count = (double)a.per_channel;
    double bl = __builtin_huge_val();
    int bk = 0x7fffffff;
    for (int k = tid; k < a.candidates; k += RS_THREADS) {              // ascending k: the strict compare keeps the first least loss
        double sum = part[k];
        for (int s = 1; s < a.slices; ++s) sum += part[(int64_t)s * a.candidates + k];
        const double l = sum / count;
        if (a.loss) a.loss[(int64_t)k * a.channels + c] = l;
        if (l < bl) { bl = l; bk = k; }
    }
    s_loss[tid] = bl; s_k[tid] = bk;
    __syncthreads();
    for (int w = RS_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w && rs_better(s_loss[tid + w], s_k[tid + w], s_loss[tid], s_k[tid])) { s_loss[tid] = s_loss[tid + w]; s_k[tid] = s_k[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) a.best[c] = s_k[0] == 0x7fffffff ? 0 : s_k[0];
}

}  // namespace

}  // namespace qv2x

extern "C" int64_t qv2x_range_search_workspace_bytes(const qv2x_range_search_desc* d) {
    using namespace qv2x;
    if (rs_check(d, "qv2x_range_search_workspace_bytes")) return -1;
    return (int64_t)d->channels * rs_shape(d).slices * d->candidates * (int64_t)sizeof(double);
}

extern "C" int qv2x_range_search_f32(const qv2x_range_search_desc* d, const float* x, const float* delta, const float* zp, double* loss,
                                     int32_t* best, void* workspace, void* stream) {
    using namespace qv2x;
    const char* who = "qv2x_range_search_f32";
    if (int rc = rs_check(d, who)) return rc;
    if (!x || !delta || !zp || !best || !workspace) return fail(QV2X_EINVAL, "%s: null pointer", who);
    if ((uintptr_t)workspace & 7) return fail(QV2X_EINVAL, "%s: workspace must be 8-byte aligned", who);
    const RsShape s = rs_shape(d);
    RsArgs a{};
    a.channels = d->channels; a.candidates = d->candidates; a.tiles = (int)s.tiles; a.slices = (int)s.slices;
    a.per_channel = d->per_channel; a.slice_len = s.chunks_per_slice * RS_CHUNK;
    a.top = (float)(d->n_levels - 1);
    a.x = x; a.delta = delta; a.zp = zp; a.partial = (double*)workspace; a.loss = loss; a.best = best;
    hipStream_t st = (hipStream_t)stream;
    rs_partial_kernel<<<dim3((unsigned)s.groups), RS_THREADS, 0, st>>>(a);
    rs_reduce_kernel<<<dim3((unsigned)d->channels), RS_THREADS, 0, st>>>(a);
    return hip_check(hipGetLastError(), who);
}
