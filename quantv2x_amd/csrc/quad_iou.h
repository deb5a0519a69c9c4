// Area of two convex quadrilaterals and of their intersection in fp64: what the rotated NMS (postprocess.hip) and the detection evaluator
// (eval.hip) both call an IoU.  The reference takes these areas from shapely (un-vendored); oracle/postprocess.py restates the clipping
// below operation for operation, and the post-process suites hold the two bit-equal; tests/test_postprocess_cases_cpu.py holds the
// clipping itself against a reference that does not clip.
#pragma once
#include "common.h"

namespace qv2x {

// area of the intersection of two convex quadrilaterals, Sutherland-Hodgman in fp64 (oracle/postprocess.py)
static __device__ double quad_inter_area(const double (&p)[4][2], const double (&q)[4][2]) {
    double qa = 0.0;
    for (int i = 0; i < 4; ++i) qa += q[i][0] * q[(i + 1) & 3][1] - q[(i + 1) & 3][0] * q[i][1];
    if (qa == 0.0) return 0.0;                                     // a clip polygon without area (a point: four zero-length edges clip nothing)
    const bool rev = qa < 0.0;                                     // clip polygon walked counter-clockwise
    double cur[8][2], nxt[8][2];
    int n = 4;
    for (int i = 0; i < 4; ++i) { cur[i][0] = p[i][0]; cur[i][1] = p[i][1]; }
    for (int e = 0; e < 4 && n > 0; ++e) {
        const int i0 = rev ? 3 - e : e, i1 = rev ? (2 - e) & 3 : (e + 1) & 3;      // reversed polygon: q3 q2 q1 q0
        const double ax = q[i0][0], ay = q[i0][1], bx = q[i1][0], by = q[i1][1];
        int m = 0;
        for (int j = 0; j < n; ++j) {
            const double cx = cur[j][0], cy = cur[j][1], dx = cur[(j + 1) % n][0], dy = cur[(j + 1) % n][1];
            const double sc = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
            const double sd = (bx - ax) * (dy - ay) - (by - ay) * (dx - ax);
            if (sc >= 0.0) { nxt[m][0] = cx; nxt[m][1] = cy; ++m; }
            if ((sc >= 0.0) != (sd >= 0.0)) {
                const double t = sc / (sc - sd);
                nxt[m][0] = cx + t * (dx - cx); nxt[m][1] = cy + t * (dy - cy); ++m;
            }
        }
        n = m;
        for (int j = 0; j < n; ++j) { cur[j][0] = nxt[j][0]; cur[j][1] = nxt[j][1]; }
    }
    if (n < 3) return 0.0;
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += cur[j][0] * cur[(j + 1) % n][1] - cur[(j + 1) % n][0] * cur[j][1];
    return fabs(0.5 * s);
}

static __device__ __forceinline__ double quad_area(const double (&q)[4][2]) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += q[i][0] * q[(i + 1) & 3][1] - q[(i + 1) & 3][0] * q[i][1];
    return fabs(0.5 * s);
}

}  // namespace qv2x
