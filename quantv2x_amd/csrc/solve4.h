// x with a x = b for 4 x 4 float64 matrices: Gaussian elimination with partial pivoting (first largest pivot), every update a separate
// multiply and subtract (the library is built with -ffp-contract=off), then back substitution.  The fixed operation order of
// oracle/geometry.py:solve4 -- bit-identical to it; equal to np.linalg.solve, the reference's call at
// opencood/utils/transformation_utils.py:60, to a few ulp.  `a` and `b` are used up.  Shared by pairwise.hip (the V2X link's 4 x 4 poses)
// and scene_prep.hip (6-DoF poses).
#pragma once

namespace qv2x {

__device__ __forceinline__ void solve4(double (&a)[4][4], double (&b)[4][4], double (&x)[4][4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int p = k;
#pragma unroll
        for (int r = k + 1; r < 4; ++r)
            if (fabs(a[r][k]) > fabs(a[p][k])) p = r;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double ta = a[k][c], tb = b[k][c];
#pragma unroll
            for (int r = k + 1; r < 4; ++r)
                if (r == p) { a[k][c] = a[r][c]; a[r][c] = ta; b[k][c] = b[r][c]; b[r][c] = tb; }
        }
#pragma unroll
        for (int r = k + 1; r < 4; ++r) {
            const double m = a[r][k] / a[k][k];
#pragma unroll
            for (int c = k + 1; c < 4; ++c) a[r][c] = a[r][c] - m * a[k][c];
#pragma unroll
            for (int c = 0; c < 4; ++c) b[r][c] = b[r][c] - m * b[k][c];
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 3; r >= 0; --r) {
            double s = b[r][c];
#pragma unroll
            for (int q = r + 1; q < 4; ++q) s = s - a[r][q] * x[q][c];
            x[r][c] = s / a[r][r];
        }
}

}  // namespace qv2x
