// Detection evaluation on the GPU: per frame and per (class, range, threshold) problem, which detections are true / false positives --
// caluclate_tp_fp of the reference (opencood/utils/eval_utils.py:40-120; eval_utils_mc.py:41-93 is the same without the range filter) for
// a whole batch, every problem at once, nothing read back.  Three kernels:
//   1. ev_rank_kernel   stable descending score order of a frame's detections by counting (<= 1024 rows: rank = how many rows come first),
//                       and the membership word of every detection (by rank) and GT: bit (class * n_ranges + range), of the low
//                       half = label and centre distance fit that problem set                                                       (eval_utils.py:80-98)
//   2. ev_iou_kernel    the fp32 IoU matrix [rank][gt] of the frame, once for all problems: (float)(inter / union) in fp64 with the
//                       clipping of the rotated NMS (quad_iou.h)                                  (common_utils.py:230-252)
//   3. ev_match_kernel  the greedy walk (eval_utils.py:100-114).  The walk over detections is serial; what runs side by side is
//                       frames x (class, range) sets, and inside a set the GT across the 64 lanes of ONE wave (gt_cap 256 = 4 per lane).
//                       The thresholds of a set read the same IoU rows: the wave carries all of them, one alive-mask per threshold.
//                       Argmax = a DPP max over the IoU bits, then ballots find the lowest GT row that holds it.  No barrier: LDS only holds
//                       what a lane itself wrote.
// Ties: equal scores keep the lower row first (np.argsort(-score) of the reference is unstable: undefined there); equal IoUs go to the
// lowest GT row (np.argmax on the list that `pop` keeps in order).
#include "common.h"
#include "quad_iou.h"

namespace qv2x {

namespace {

constexpr int EV_MAX_FRAMES = 64, EV_DET_MAX = 1024, EV_GT_MAX = 256, EV_SLOTS = EV_GT_MAX / 64;

struct EvArgs {
    int frames, det_cap, gt_cap, n_classes, n_ranges, n_thr;
    float ranges[4][2], thr[4];
    const float* det_corners; const float* det_scores; const int* det_labels; const int* det_count;
    const float* gt_corners; const int* gt_labels; const int* gt_count;
    float* iou; unsigned* det_member; unsigned* gt_member;                         // workspace: [frames][det_cap][gt_cap], [frames][det_cap] by RANK (low half: member of the set, high half: overlaps a GT of it), [frames][gt_cap]
    int* out_order; float* out_scores; unsigned char* out_flags; int* out_match; int* out_gt;
};

__device__ __forceinline__ int ev_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// bit (c * n_ranges + g) of the result: the box (label `label`, corners c[8][3]) belongs to the problems of class c + 1 and range g
__device__ __forceinline__ unsigned ev_member(const EvArgs& a, const float* c, int label) {
    const double cx = ((double)c[0] + (double)c[3] + (double)c[6] + (double)c[9]) * 0.25;      // centre of the bottom face: corners 0..3 in index order
    const double cy = ((double)c[1] + (double)c[4] + (double)c[7] + (double)c[10]) * 0.25;
    const double d = sqrt(cx * cx + cy * cy);
    unsigned in_range = 0u;
    for (int g = 0; g < a.n_ranges; ++g)
        if ((double)a.ranges[g][0] < d && d < (double)a.ranges[g][1]) in_range |= 1u << g;
    if (a.n_classes == 0) return in_range;
    if (label < 1 || label > a.n_classes) return 0u;                 // a label outside 1..n_classes belongs to no problem
    return in_range << ((label - 1) * a.n_ranges);
}

// grid (det_cap / 256, frames)
__global__ __launch_bounds__(256) void ev_rank_kernel(const EvArgs a) {
    __shared__ float s[EV_DET_MAX];
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int count = ev_clamp(a.det_count[f], a.det_cap), gc = ev_clamp(a.gt_count[f], a.gt_cap);
    const float* sc = a.det_scores + (size_t)f * a.det_cap;
    for (int j = threadIdx.x; j < count; j += 256) s[j] = sc[j];
    __syncthreads();
    if (i < a.det_cap) {
        const size_t o = (size_t)f * a.det_cap;
        if (i < count) {
            const float mine = s[i];
            int rank = 0;
            for (int j = 0; j < count; ++j) {
                const float v = s[j];
                rank += (v > mine) | ((v == mine) & (j < i));
            }
            a.out_order[o + rank] = i;
            a.out_scores[o + rank] = mine;
            a.det_member[o + rank] = ev_member(a, a.det_corners + (o + i) * 24, a.det_labels ? a.det_labels[o + i] : 0);
        } else {                                                      // the ranks past the frame's detections
            a.out_order[o + i] = -1;
            a.out_scores[o + i] = 0.0f;
            a.det_member[o + i] = 0u;
        }
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < a.gt_cap) {
        const int g = threadIdx.x;
        const size_t o = (size_t)f * a.gt_cap + g;
        a.gt_member[o] = g < gc ? ev_member(a, a.gt_corners + o * 24, a.gt_labels ? a.gt_labels[o] : 0) : 0u;
    }
}

__device__ __forceinline__ void ev_load_quad(const float* c, double (&q)[4][2]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { q[k][0] = (double)c[k * 3]; q[k][1] = (double)c[k * 3 + 1]; }
}

// grid (det_cap * gt_cap / 256, frames): thread e of a frame = (rank e / gt_count, GT e % gt_count)
__global__ __launch_bounds__(256) void ev_iou_kernel(const EvArgs a) {
    const int f = blockIdx.y;
    const int count = ev_clamp(a.det_count[f], a.det_cap), gc = ev_clamp(a.gt_count[f], a.gt_cap);
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (gc == 0 || e >= count * gc) return;
    const int r = e / gc, g = e - r * gc;
    int row = a.out_order[(size_t)f * a.det_cap + r];
    if ((unsigned)row >= (unsigned)count) row = 0;                    // (non-finite scores: the order is undefined, the addresses are not)
    double qi[4][2], qj[4][2];
    ev_load_quad(a.det_corners + ((size_t)f * a.det_cap + row) * 24, qi);
    ev_load_quad(a.gt_corners + ((size_t)f * a.gt_cap + g) * 24, qj);
    double ix0 = qi[0][0], ix1 = qi[0][0], iy0 = qi[0][1], iy1 = qi[0][1], jx0 = qj[0][0], jx1 = qj[0][0], jy0 = qj[0][1], jy1 = qj[0][1];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        ix0 = fmin(ix0, qi[k][0]); ix1 = fmax(ix1, qi[k][0]); iy0 = fmin(iy0, qi[k][1]); iy1 = fmax(iy1, qi[k][1]);
        jx0 = fmin(jx0, qj[k][0]); jx1 = fmax(jx1, qj[k][0]); jy0 = fmin(jy0, qj[k][1]); jy1 = fmax(jy1, qj[k][1]);
    }
    const bool apart = ix1 < jx0 || jx1 < ix0 || iy1 < jy0 || jy1 < iy0;         // disjoint bounding boxes: intersection 0 (as pp_iou_kernel)
    const double inter = apart ? 0.0 : quad_inter_area(qi, qj);
    const double uni = quad_area(qi) + quad_area(qj) - inter;
    const float v = uni > 0.0 ? (float)(inter / uni) : 0.0f;
    a.iou[((size_t)f * a.det_cap + r) * a.gt_cap + g] = v;
    // the rank's word, high half: the sets in which it overlaps a GT at all (an OR: no order to decide); the walk visits only those
    if (v > 0.0f) atomicOr(&a.det_member[(size_t)f * a.det_cap + r], a.gt_member[(size_t)f * a.gt_cap + g] << 16);
}

// max over the wave of an unsigned value (every lane gets it): quad, half-row and row steps by DPP, the four rows by readlane
__device__ __forceinline__ unsigned ev_umax(unsigned x, unsigned y) { return x > y ? x : y; }
__device__ __forceinline__ unsigned wave_max_u32(unsigned x) {
    x = ev_umax(x, (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xf, 0xf, true));      // quad_perm [1,0,3,2]
    x = ev_umax(x, (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xf, 0xf, true));      // quad_perm [2,3,0,1]
    x = ev_umax(x, (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0x141, 0xf, 0xf, true));     // row_half_mirror
    x = ev_umax(x, (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0x140, 0xf, 0xf, true));     // row_mirror
    return ev_umax(ev_umax((unsigned)__builtin_amdgcn_readlane((int)x, 0), (unsigned)__builtin_amdgcn_readlane((int)x, 16)),
                   ev_umax((unsigned)__builtin_amdgcn_readlane((int)x, 32), (unsigned)__builtin_amdgcn_readlane((int)x, 48)));
}

// One wave per (class, range) set of a frame: grid (sets, frames), 64 threads.  Lane l holds GT rows l, 64 + l, 128 + l, 192 + l (slot k =
// row 64 k + l); alive[t] bit k = that GT is in the set and not yet matched at threshold t.  An IoU is >= +0, so its bit pattern orders
// like its value.  Ranks are walked 64 at a time: lane i keeps the results of rank 64 c + i and stores them at the end of the chunk; only
// the chunk's members that overlap a GT of the set at all cost a step (the IoU kernel marks them in the high half of the rank's word; every
// other member is a false positive at every threshold).  A step's IoU row comes from LDS, where the walk's rows were put sixteen at a
// time: a global load per step kept the walk waiting on memory.  A lone wave issues one instruction every four cycles or so whatever its
// kind, so a step costs what it counts in instructions.  Measured at 32 frames x 1000 detections x 100 GT, 3 thresholds x 4 ranges
// (tools/bench_eval.py): a global load per step 726 us; rows from LDS 570 us; only overlapping members walked 366 us (this form); the
// thresholds' reductions unrolled side by side without the `if (tp)` branch 468 us; alive masks as ballot words on the scalar unit and the
// overlapping GT visited one by one 417 us.
__global__ __launch_bounds__(64) void ev_match_kernel(const EvArgs a) {
    const int f = blockIdx.y, set = blockIdx.x, lane = threadIdx.x;
    const int count = ev_clamp(a.det_count[f], a.det_cap), gc = ev_clamp(a.gt_count[f], a.gt_cap);
    const int K = (gc + 63) >> 6;
    const int nthr = a.n_thr;
    const size_t P = (size_t)gridDim.x * nthr;
    unsigned mine = 0u;
    int ngt = 0;
#pragma unroll
    for (int k = 0; k < EV_SLOTS; ++k) {
        const int g = 64 * k + lane;
        const bool in = g < gc && ((a.gt_member[(size_t)f * a.gt_cap + g] >> set) & 1u);
        mine |= in ? 1u << k : 0u;
        ngt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(in));
    }
    unsigned alive[4] = {mine, mine, mine, mine};
    if (lane < nthr) a.out_gt[(size_t)f * P + (size_t)set * nthr + lane] = ngt;
    const float* iou_f = a.iou + (size_t)f * a.det_cap * a.gt_cap;
    const unsigned* words = a.det_member + (size_t)f * a.det_cap;
    __shared__ unsigned rows[64][EV_GT_MAX];                          // the chunk's IoU rows; lane l writes and reads columns 64 k + l only: no barrier
    unsigned wnext = lane < count ? words[lane] : 0u;
    for (int c0 = 0; c0 < a.det_cap; c0 += 64) {
        const unsigned w = wnext;                                     // rank c0 + lane (0 past the frame's count); the next chunk's is requested now
        wnext = c0 + 64 + lane < count ? words[c0 + 64 + lane] : 0u;
        const bool member = (w >> set) & 1u;
        int fl[4], mt[4] = {-1, -1, -1, -1};
#pragma unroll
        for (int t = 0; t < 4; ++t) fl[t] = (member && t < nthr) ? 1 : 0;      // (what the walk does not visit overlaps no GT of the set)
        unsigned long long todo = __builtin_amdgcn_ballot_w64(member && ((w >> (16 + set)) & 1u)), walk = todo;
        while (todo) {                                                // (wave-uniform) the rows of the walk into LDS, sixteen requested together
            int idx[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                idx[q] = todo ? __builtin_ctzll(todo) : -1;
                todo &= todo - 1ull;                                  // (0 stays 0)
            }
            unsigned v[16][EV_SLOTS];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float* row = iou_f + (size_t)(c0 + (idx[q] >= 0 ? idx[q] : 0)) * a.gt_cap;      // (a walked rank is below the frame's count)
#pragma unroll
                for (int k = 0; k < EV_SLOTS; ++k)
                    v[q][k] = (idx[q] >= 0 && k < K && 64 * k + lane < gc) ? __builtin_bit_cast(unsigned, row[64 * k + lane]) : 0u;
            }
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (idx[q] >= 0) {
#pragma unroll
                    for (int k = 0; k < EV_SLOTS; ++k) rows[idx[q]][64 * k + lane] = v[q][k];
                }
        }
        while (walk) {                                                // (wave-uniform)
            const int b = __builtin_ctzll(walk);
            walk &= walk - 1ull;
            unsigned cur[EV_SLOTS];
#pragma unroll
            for (int k = 0; k < EV_SLOTS; ++k) cur[k] = rows[b][64 * k + lane];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t >= nthr) break;
                unsigned best = 0u;
#pragma unroll
                for (int k = 0; k < EV_SLOTS; ++k) best = ((alive[t] >> k) & 1u) ? ev_umax(best, cur[k]) : best;
                const bool any = __builtin_amdgcn_ballot_w64(alive[t] != 0u) != 0ull;
                const unsigned m = wave_max_u32(best);
                const bool tp = any && !(__builtin_bit_cast(float, m) < a.thr[t]);        // FP: no GT left, or the largest IoU below the threshold (fp32)
                int row = -1;
                if (tp) {                                             // (wave-uniform) the lowest row that holds the maximum: lowest slot, then lowest lane
                    for (int k = 0; k < K; ++k) {
                        const unsigned long long hit = __builtin_amdgcn_ballot_w64(((alive[t] >> k) & 1u) && cur[k] == m);
                        if (hit) {
                            const int l = __builtin_ctzll(hit);
                            row = 64 * k + l;
                            if (lane == l) alive[t] &= ~(1u << k);
                            break;
                        }
                    }
                }
                if (lane == b) { fl[t] = tp ? 2 : 1; mt[t] = row; }
            }
        }
        const int r = c0 + lane;
        if (r < a.det_cap) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t >= nthr) break;
                const size_t o = ((size_t)f * P + (size_t)set * nthr + t) * a.det_cap + r;
                a.out_flags[o] = (unsigned char)fl[t];
                a.out_match[o] = mt[t];
            }
        }
    }
}

size_t ev_align(size_t v) { return (v + 255) & ~(size_t)255; }
struct EvLayout { size_t iou, det_member, gt_member, total; };
EvLayout ev_layout(const qv2x_eval_desc* d) {
    EvLayout l{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = ev_align(o + bytes); return at; };
    l.iou = take((size_t)d->frames * d->det_cap * d->gt_cap * 4);
    l.det_member = take((size_t)d->frames * d->det_cap * 4);
    l.gt_member = take((size_t)d->frames * d->gt_cap * 4);
    l.total = o;
    return l;
}

int ev_check(const qv2x_eval_desc* d, const char* who) {
    if (!d) return fail(QV2X_EINVAL, "%s: null descriptor", who);
    if (d->frames < 1 || d->frames > EV_MAX_FRAMES) return fail(QV2X_EINVAL, "%s: 1..%d frames", who, EV_MAX_FRAMES);
    if (d->det_cap < 1 || d->det_cap > EV_DET_MAX) return fail(QV2X_EINVAL, "%s: det_cap in 1..%d", who, EV_DET_MAX);
    if (d->gt_cap < 1 || d->gt_cap > EV_GT_MAX) return fail(QV2X_EINVAL, "%s: gt_cap in 1..%d", who, EV_GT_MAX);
    if (d->n_classes < 0 || d->n_classes > 4) return fail(QV2X_EINVAL, "%s: n_classes in 0..4", who);
    if (d->n_ranges < 1 || d->n_ranges > 4) return fail(QV2X_EINVAL, "%s: n_ranges in 1..4", who);
    if (d->n_thresholds < 1 || d->n_thresholds > 4) return fail(QV2X_EINVAL, "%s: n_thresholds in 1..4", who);
    for (int t = 0; t < d->n_thresholds; ++t)
        if (!(d->thresholds[t] > 0.0f && d->thresholds[t] <= 1.0f)) return fail(QV2X_EINVAL, "%s: threshold %d outside (0, 1]", who, t);
    for (int g = 0; g < d->n_ranges; ++g)
        if (d->ranges[g][0] != d->ranges[g][0] || d->ranges[g][1] != d->ranges[g][1]) return fail(QV2X_EINVAL, "%s: range %d is not a number", who, g);
    return QV2X_OK;
}

}  // namespace

}  // namespace qv2x

extern "C" int64_t qv2x_eval_workspace_bytes(const qv2x_eval_desc* d) {
    using namespace qv2x;
    if (ev_check(d, "qv2x_eval_workspace_bytes")) return -1;
    return (int64_t)ev_layout(d).total;
}

extern "C" int qv2x_eval_tp_fp_f32(const qv2x_eval_desc* d, const float* det_corners, const float* det_scores, const int32_t* det_labels,
                                   const int32_t* det_count, const float* gt_corners, const int32_t* gt_labels, const int32_t* gt_count,
                                   void* workspace, int64_t workspace_bytes, int32_t* out_order, float* out_scores, uint8_t* out_flags,
                                   int32_t* out_match, int32_t* out_gt, void* stream) {
    using namespace qv2x;
    const char* who = "qv2x_eval_tp_fp_f32";
    if (int rc = ev_check(d, who)) return rc;
    if (!det_corners || !det_scores || !det_count || !gt_corners || !gt_count || !workspace || !out_order || !out_scores || !out_flags ||
        !out_match || !out_gt)
        return fail(QV2X_EINVAL, "%s: null pointer", who);
    if (d->n_classes > 0 && (!det_labels || !gt_labels)) return fail(QV2X_EINVAL, "%s: n_classes > 0 needs det_labels and gt_labels", who);
    const EvLayout l = ev_layout(d);
    if (workspace_bytes < (int64_t)l.total) return fail(QV2X_EINVAL, "%s: workspace of %lld bytes, need %lld", who, (long long)workspace_bytes, (long long)l.total);
    if ((uintptr_t)workspace & 255) return fail(QV2X_EALIGN, "%s: workspace must be 256-byte aligned", who);
    char* ws = (char*)workspace;
    EvArgs a{};
    a.frames = d->frames; a.det_cap = d->det_cap; a.gt_cap = d->gt_cap; a.n_classes = d->n_classes; a.n_ranges = d->n_ranges; a.n_thr = d->n_thresholds;
    for (int g = 0; g < 4; ++g) { a.ranges[g][0] = d->ranges[g][0]; a.ranges[g][1] = d->ranges[g][1]; a.thr[g] = d->thresholds[g]; }
    a.det_corners = det_corners; a.det_scores = det_scores; a.det_labels = d->n_classes > 0 ? det_labels : nullptr; a.det_count = det_count;
    a.gt_corners = gt_corners; a.gt_labels = d->n_classes > 0 ? gt_labels : nullptr; a.gt_count = gt_count;
    a.iou = (float*)(ws + l.iou); a.det_member = (unsigned*)(ws + l.det_member); a.gt_member = (unsigned*)(ws + l.gt_member);
    a.out_order = out_order; a.out_scores = out_scores; a.out_flags = out_flags; a.out_match = out_match; a.out_gt = out_gt;
    hipStream_t st = (hipStream_t)stream;
    const unsigned F = (unsigned)d->frames, sets = (unsigned)((d->n_classes > 0 ? d->n_classes : 1) * d->n_ranges);
    ev_rank_kernel<<<dim3((unsigned)((d->det_cap + 255) / 256), F), 256, 0, st>>>(a);
    ev_iou_kernel<<<dim3((unsigned)((d->det_cap * d->gt_cap + 255) / 256), F), 256, 0, st>>>(a);
    ev_match_kernel<<<dim3(sets, F), 64, 0, st>>>(a);
    return hip_check(hipGetLastError(), who);
}
