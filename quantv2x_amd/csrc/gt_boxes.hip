// Ground-truth boxes on the GPU: generate_gt_bbx / generate_gt_bbx_by_iou of the reference (opencood/data_utils/post_processor/
// base_postprocessor.py:47-107, :110-200; base_postprocessor_multi_class.py:46-103) for a whole batch, in the layout the detection
// evaluator (eval.hip) reads, nothing read back.  One kernel, one workgroup of 256 threads per frame (the frame is the grid dimension):
//   1. the frame's candidate flags (row of a used agent with its mask set) and ids into LDS; row r = agent * obj_cap + slot, so row order
//      is the reference's concatenation order;
//   2. mode 1 only: the projected bottom faces of the candidates into LDS (the IoU filter compares PROJECTED boxes);
//   3. rows in rounds of 256, four waves of 64 in row order.  A row survives iff it is a candidate and (mode 0) no earlier candidate has
//      its id -- a plain compare against all earlier rows out of LDS, 2048 rows at most -- or (mode 1) it belongs to agent 0, or to agent 1
//      and its IoU with every candidate of agent 0 is <= the threshold.  Only then the survivor's OWN box is range-masked (the reference's
//      order: an id whose first occurrence lies out of range is gone, whatever a later copy of it looks like);
//   4. stable compaction of the round: wave ballot + popcount below the lane, the four wave totals through LDS, the running count of the
//      earlier rounds in a register every thread carries.  The survivors land in candidate order; rows past gt_cap are counted, not written.
// Corners: the f32 inputs in fp64 -- half extents times the template of box_utils.boxes_to_corners_3d (:193-196), the rotation of
// common_utils.rotate_points_along_z (:139-161), plus the centre, then rows 0..2 of the 4x4 transform (box_utils.project_box3d :278-316) --
// rounded to f32 ONCE; the range decision is taken on that f32 value against the f32 bounds (>= and <=, box_utils.py:348-421).
// The library is built with -ffp-contract=off: the sums below are evaluated as written.
#include "common.h"
#include "quad_iou.h"

namespace qv2x {

namespace {

constexpr int GT_MAX_FRAMES = 64, GT_MAX_AGENTS = 8, GT_OBJ_MAX = 256, GT_CAP_MAX = 256, GT_ROWS_MAX = GT_MAX_AGENTS * GT_OBJ_MAX;
constexpr int GT_THREADS = 256, GT_WAVES = GT_THREADS / 64;

struct GtArgs {
    int agents, obj_cap, gt_cap, row_floats, order, mode, xy_only;
    float range[6], thr;
    const float* boxes; const unsigned char* mask; const int* ids; const float* tf; const int* agent_counts;
    float* out_corners; int* out_labels; int* out_ids; int* out_counts; int* out_totals;
};

// the 8 corners of one box row in the ego frame, f32 (rounded once)
__device__ __forceinline__ void gt_project(const GtArgs& a, const float* b, const float* T, float (&c)[8][3]) {
    const double cx = (double)b[0], cy = (double)b[1], cz = (double)b[2];
    const double hl = 0.5 * (double)b[a.order == 0 ? 5 : 3], hw = 0.5 * (double)b[4], hh = 0.5 * (double)b[a.order == 0 ? 3 : 5];   // 'hwl' rows are permuted to l, w, h
    const double yaw = (double)b[6], cs = cos(yaw), sn = sin(yaw);
    double t[3][4];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) t[i][j] = (double)T[i * 4 + j];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int q = k & 3;                                          // template: (1,-1) (1,1) (-1,1) (-1,-1), bottom face first
        const double x = (q < 2 ? hl : -hl), y = ((q == 1 || q == 2) ? hw : -hw), z = (k < 4 ? -hh : hh);
        const double xr = (x * cs - y * sn) + cx, yr = (x * sn + y * cs) + cy, zr = z + cz;
#pragma unroll
        for (int i = 0; i < 3; ++i) c[k][i] = (float)(((t[i][0] * xr + t[i][1] * yr) + t[i][2] * zr) + t[i][3]);
    }
}

__device__ __forceinline__ bool gt_in_range(const GtArgs& a, const float (&c)[8][3]) {
    bool in = true;
    const int dims = a.xy_only ? 2 : 3;
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (i < dims) in = in && c[k][i] >= a.range[i] && c[k][i] <= a.range[3 + i];
    return in;
}

// (float)(inter / union) of two bottom faces, as ev_iou_kernel
__device__ float gt_iou(const double (&qi)[4][2], const double (&qj)[4][2]) {
    double ix0 = qi[0][0], ix1 = qi[0][0], iy0 = qi[0][1], iy1 = qi[0][1], jx0 = qj[0][0], jx1 = qj[0][0], jy0 = qj[0][1], jy1 = qj[0][1];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        ix0 = fmin(ix0, qi[k][0]); ix1 = fmax(ix1, qi[k][0]); iy0 = fmin(iy0, qi[k][1]); iy1 = fmax(iy1, qi[k][1]);
        jx0 = fmin(jx0, qj[k][0]); jx1 = fmax(jx1, qj[k][0]); jy0 = fmin(jy0, qj[k][1]); jy1 = fmax(jy1, qj[k][1]);
    }
    const bool apart = ix1 < jx0 || jx1 < ix0 || iy1 < jy0 || jy1 < iy0;
    const double inter = apart ? 0.0 : quad_inter_area(qi, qj);
    const double uni = quad_area(qi) + quad_area(qj) - inter;
    return uni > 0.0 ? (float)(inter / uni) : 0.0f;
}

// grid (frames), 256 threads
__global__ __launch_bounds__(GT_THREADS) void gt_boxes_kernel(const GtArgs a) {
    __shared__ __attribute__((aligned(16))) int s_id[GT_ROWS_MAX];
    __shared__ __attribute__((aligned(16))) unsigned char s_cand[GT_ROWS_MAX];
    __shared__ float s_quad[2 * GT_OBJ_MAX][8];                       // mode 1: x, y of corners 0..3 of the projected candidates (agents <= 2)
    __shared__ int s_wave[GT_WAVES];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = a.agents * a.obj_cap;
    int used = a.agent_counts[f];
    used = used < 0 ? 0 : (used > a.agents ? a.agents : used);
    const int live = used * a.obj_cap;                                // rows of the agents in use: nothing past them is read
    const size_t row0 = (size_t)f * R;
    const float* tf = a.tf + (size_t)f * a.agents * 16;
    for (int r = tid; r < R; r += GT_THREADS) {
        const bool cand = r < live && a.mask[row0 + r] != 0;
        s_cand[r] = cand ? 1 : 0;
        s_id[r] = (cand && a.mode == 0) ? a.ids[row0 + r] : 0;
        if (cand && a.mode == 1) {
            float c[8][3];
            gt_project(a, a.boxes + (row0 + r) * a.row_floats, tf + (r / a.obj_cap) * 16, c);
#pragma unroll
            for (int k = 0; k < 4; ++k) { s_quad[r][2 * k] = c[k][0]; s_quad[r][2 * k + 1] = c[k][1]; }
        }
    }
    __syncthreads();
    int run = 0;                                                      // survivors of the earlier rounds (the same in every thread)
    for (int r0 = 0; r0 < live; r0 += GT_THREADS) {
        const int r = r0 + tid;
        bool keep = r < live && s_cand[r] != 0;
        if (keep && a.mode == 0) {
            const int id = s_id[r];
            bool dup = false;
            int j = 0;
            for (; j + 4 <= r && !dup; j += 4) {                      // four earlier rows per step
                const int4 v = *reinterpret_cast<const int4*>(&s_id[j]);
                const unsigned m = *reinterpret_cast<const unsigned*>(&s_cand[j]);
                dup = ((m & 0xffu) && v.x == id) || ((m & 0xff00u) && v.y == id) || ((m & 0xff0000u) && v.z == id) || ((m & 0xff000000u) && v.w == id);
            }
            for (; j < r && !dup; ++j) dup = s_cand[j] != 0 && s_id[j] == id;
            keep = !dup;
        } else if (keep && a.mode == 1 && r >= a.obj_cap) {           // the second label source: dropped when it overlaps a box of the first
            double qi[4][2], qj[4][2];
#pragma unroll
            for (int k = 0; k < 4; ++k) { qi[k][0] = (double)s_quad[r][2 * k]; qi[k][1] = (double)s_quad[r][2 * k + 1]; }
            for (int j = 0; j < a.obj_cap && keep; ++j) {
                if (!s_cand[j]) continue;
#pragma unroll
                for (int k = 0; k < 4; ++k) { qj[k][0] = (double)s_quad[j][2 * k]; qj[k][1] = (double)s_quad[j][2 * k + 1]; }
                keep = !(gt_iou(qi, qj) > a.thr);
            }
        }
        float c[8][3];
        if (keep) {
            gt_project(a, a.boxes + (row0 + r) * a.row_floats, tf + (r / a.obj_cap) * 16, c);
            keep = gt_in_range(a, c);
        }
        const unsigned long long vote = __builtin_amdgcn_ballot_w64(keep);
        if (lane == 0) s_wave[wave] = __builtin_popcountll(vote);
        __syncthreads();
        int before = run, total = 0;
#pragma unroll
        for (int w = 0; w < GT_WAVES; ++w) {
            const int n = s_wave[w];
            before += w < wave ? n : 0;
            total += n;
        }
        const int pos = before + __builtin_popcountll(vote & ((1ull << lane) - 1ull));
        if (keep && pos < a.gt_cap) {
            const size_t o = (size_t)f * a.gt_cap + pos;
            float* dst = a.out_corners + o * 24;
#pragma unroll
            for (int k = 0; k < 8; ++k)
#pragma unroll
                for (int i = 0; i < 3; ++i) dst[k * 3 + i] = c[k][i];
            if (a.out_labels) a.out_labels[o] = (int)a.boxes[(row0 + r) * a.row_floats + 7];
            if (a.out_ids) a.out_ids[o] = a.mode == 0 ? s_id[r] : r;
        }
        run += total;
        __syncthreads();                                              // s_wave is written again in the next round
    }
    if (tid == 0) {
        a.out_counts[f] = run < a.gt_cap ? run : a.gt_cap;
        a.out_totals[f] = run;
    }
}

int gt_check(const qv2x_gt_desc* d, const char* who) {
    if (!d) return fail(QV2X_EINVAL, "%s: null descriptor", who);
    if (d->frames < 1 || d->frames > GT_MAX_FRAMES) return fail(QV2X_EINVAL, "%s: 1..%d frames", who, GT_MAX_FRAMES);
    if (d->agents < 1 || d->agents > GT_MAX_AGENTS) return fail(QV2X_EINVAL, "%s: 1..%d agents", who, GT_MAX_AGENTS);
    if (d->obj_cap < 1 || d->obj_cap > GT_OBJ_MAX) return fail(QV2X_EINVAL, "%s: obj_cap in 1..%d", who, GT_OBJ_MAX);
    if (d->gt_cap < 1 || d->gt_cap > GT_CAP_MAX) return fail(QV2X_EINVAL, "%s: gt_cap in 1..%d", who, GT_CAP_MAX);
    if (d->row_floats != 7 && d->row_floats != 8) return fail(QV2X_EINVAL, "%s: row_floats 7 or 8", who);
    if (d->order != 0 && d->order != 1) return fail(QV2X_EINVAL, "%s: order 0 (hwl) or 1 (lwh)", who);
    if (d->mode != 0 && d->mode != 1) return fail(QV2X_EINVAL, "%s: mode 0 (by id) or 1 (by IoU)", who);
    if (d->mode == 1 && d->agents > 2) return fail(QV2X_EINVAL, "%s: mode 1 takes at most 2 agents", who);
    if (d->range_xy_only != 0 && d->range_xy_only != 1) return fail(QV2X_EINVAL, "%s: range_xy_only 0 or 1", who);
    for (int i = 0; i < 6; ++i)
        if (d->range[i] != d->range[i]) return fail(QV2X_EINVAL, "%s: range %d is not a number", who, i);
    if (d->mode == 1 && !(d->iou_threshold >= 0.0f && d->iou_threshold <= 1.0f)) return fail(QV2X_EINVAL, "%s: iou_threshold outside [0, 1]", who);
    return QV2X_OK;
}

}  // namespace

}  // namespace qv2x

extern "C" int qv2x_gt_boxes_f32(const qv2x_gt_desc* d, const float* boxes, const uint8_t* mask, const int32_t* ids, const float* transforms,
                                 const int32_t* agent_counts, float* gt_corners, int32_t* gt_labels, int32_t* gt_ids, int32_t* gt_counts,
                                 int32_t* gt_totals, void* stream) {
    using namespace qv2x;
    const char* who = "qv2x_gt_boxes_f32";
    if (int rc = gt_check(d, who)) return rc;
    if (!boxes || !mask || !transforms || !agent_counts || !gt_corners || !gt_counts || !gt_totals) return fail(QV2X_EINVAL, "%s: null pointer", who);
    if (d->mode == 0 && !ids) return fail(QV2X_EINVAL, "%s: mode 0 needs ids", who);
    if (d->row_floats == 8 && !gt_labels) return fail(QV2X_EINVAL, "%s: row_floats 8 needs gt_labels", who);
    GtArgs a{};
    a.agents = d->agents; a.obj_cap = d->obj_cap; a.gt_cap = d->gt_cap; a.row_floats = d->row_floats; a.order = d->order; a.mode = d->mode;
    a.xy_only = d->range_xy_only;
    for (int i = 0; i < 6; ++i) a.range[i] = d->range[i];
    a.thr = d->iou_threshold;
    a.boxes = boxes; a.mask = mask; a.ids = ids; a.tf = transforms; a.agent_counts = agent_counts;
    a.out_corners = gt_corners; a.out_labels = d->row_floats == 8 ? gt_labels : nullptr; a.out_ids = gt_ids; a.out_counts = gt_counts; a.out_totals = gt_totals;
    gt_boxes_kernel<<<dim3((unsigned)d->frames), GT_THREADS, 0, (hipStream_t)stream>>>(a);
    return hip_check(hipGetLastError(), who);
}
