// a6, stage 1 of the two-stage EXACT encode for SEGMENTED and 256-entry codebooks (seg_num 1 | 2, dict_size <= 256): the kernel of
// codebook_encode_cand.hip (read its header first: the collapsed form, the fixed-point grid, the bound) with three differences.
//   * The scores of a level are the ke = segs * kc rows of the EXTENDED codebook (segment s: rows s kc .., include/qv2x.h): ke / 32 score
//     tiles per level (48 in all at (2, 256)), and a running (best, second) PER SEGMENT, closed after the segment's kc / 32 tiles.  A
//     comparison never crosses segments.
//   * The packed score is 256 S + k (an 8-bit index); encode_two_stage.candidate_tables keeps |bias| < 2^43 so that the packed scores AND
//     their differences stay exact integers below 2^53.
//   * An earlier level subtracted one codeword PER SEGMENT, so level l adds segs * l table rows to every score (four at level 2 of two
//     segments): row s' kc + code_{j, s'} of table (l, j), [ke][ke] i32 -- 3 MB at (2, 256), L2 resident, fetched by buffer loads with one
//     32-bit lane offset each, a group ahead of their use.  The i32 bracket 256 a1 + a0 + (up to four entries) holds because the entries are
//     below 2^29 / max(2, segs * (levels - 1)).
// Codes go to plane l * segs + s; the three lists mean what they mean there (the LEVEL a cell is first undecided at: any of its segments).
//
// Cell tiles per wave (CT): the table prefetch is 2 slots x (2 segs) rows x CT x 4 registers, twice the one-segment kernel's, beside
// 3 limbs x CT x 16 accumulators and 32 CT registers of cells -- so two segments run CT = 3 at the batch (96 cells per wave share the
// 1.15 MB of limbs a wave streams), one segment of 256 codes CT = 4; both CT = 2 for small launches.  Registers and scratch: DESIGN.md §3.1.
//
// KEEP IN STEP with codebook_encode_cand.hip: the structure (cells as B fragments, the limb ring, the group-ahead prefetch of bias and
// table rows, the list reservation) is that kernel's, whose entry keeps its own kernel because its contract and launches must not move;
// the reasons for those choices, with their measurements, are in its comments and are not repeated as this kernel's own here.
#include "common.h"

namespace qv2x {
namespace {

constexpr int QV2X_CAND_SEG_CT1 = 4, QV2X_CAND_SEG_CT2 = 3;      // cell tiles per wave at the batch: one | two segments

struct CandSegArgs {
    const int8_t* in; const int8_t* gpack; const double* bias; const int* tables;
    uint8_t* codes; unsigned* list; unsigned* counters;
    float tau[3][3];
    int n, h, w, hw, M, levels, kc, ke, zx, gbytes, tbytes;
    float delta;
};

constexpr int NPF = 8;                                               // A fragments (1 KiB each) in flight ahead of the MFMAs
constexpr int LIMBS = 3;
template <int V> struct IC { static constexpr int value = V; };

__device__ __forceinline__ double shfl_xor_f64(double v, int m) {
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __shfl_xor((int)b, m), hi = __shfl_xor((int)(b >> 32), m);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}

// CT = 32-cell B tiles per wave: every A fragment feeds CT MFMAs; SEGS = seg_num.
template <int CT, int SEGS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void encode_candidates_seg_kernel(const CandSegArgs a) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 31, hf = lane >> 5;
    const int m0 = ((int)blockIdx.x * 4 + wave) * (32 * CT);
    // (a wave past the last cell walks on with clamped cells and stores nothing: the workgroup meets at a barrier at the end)

    // ---- the wave's 32 CT cells: B fragments straight from the padded map, and the two sums the bound needs ---------------------------------
    v4i xb[CT][8];
    int m[CT];
    float n0[CT], n1[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        m[ct] = m0 + 32 * ct + j;
        const int mc = m[ct] < a.M ? m[ct] : a.M - 1;
        const int img = mc / a.hw, rem = mc - img * a.hw, y = rem / a.w, x = rem - y * a.w;
        const int8_t* px = a.in + ((size_t)(img * (a.h + 2) + y + 1) * (a.w + 2) + x + 1) * 256 + 16 * hf;
#pragma unroll
        for (int s = 0; s < 8; ++s) xb[ct][s] = *(const v4i*)(px + 32 * s);
        unsigned s1 = 0, s2 = 0, sad = 0;
        const unsigned zx4 = (unsigned)a.zx * 0x01010101u;
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const unsigned u = (unsigned)xb[ct][s][d] ^ 0x80808080u;   // stored byte = code - 128
                s1 = __builtin_amdgcn_udot4(u, 0x01010101u, s1, false);
                s2 = __builtin_amdgcn_udot4(u, u, s2, false);
                sad = __builtin_amdgcn_sad_u8(u, zx4, sad);
            }
        s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32); sad += __shfl_xor(sad, 32);
        const int n2 = (int)s2 - 2 * a.zx * (int)s1 + 256 * a.zx * a.zx;    // sum (code - zx)^2 <= 256 * 255^2 < 2^24: exact as a float
        n0[ct] = a.delta * sqrtf((float)n2);
        n1[ct] = (float)sad;
    }

    const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc((void*)a.gpack, 0, a.gbytes, 0x00020000);   // past the end: zeros
    int wo = 0;
    const int loff = lane * 16;
    auto gload = [&](int f) __attribute__((always_inline)) { return (v4i)__builtin_amdgcn_raw_buffer_load_b128(grs, loff, wo + f * 1024, 0); };
    v4i ring[NPF];
#pragma unroll
    for (int i = 0; i < NPF; ++i) ring[i] = gload(i);

    // bias and table rows by buffer loads too: a scalar offset per (level, tile, group), ONE 32-bit lane offset per cell -- no 64-bit
    // per-lane address arithmetic (as in codebook_encode_cand.hip, where plain pointers spilled)
    const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc((void*)a.bias, 0, a.levels * a.ke * 8, 0x00020000);
    const __amdgpu_buffer_rsrc_t trs = __builtin_amdgcn_make_buffer_rsrc((void*)a.tables, 0, a.tbytes, 0x00020000);
    int o[2][SEGS][CT] = {};                                         // byte offsets of the cells' table rows: ((s' kc + code_{j, s'}) * ke + 4 hf) * 4
    int first[CT];                                                   // the level a cell is first undecided at (3: never)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) first[ct] = 3;
    const int ntile = a.kc >> 5;                                     // score tiles per segment
    const int tsz = a.ke * a.ke;                                     // entries of one table
    auto level = [&](auto lc) __attribute__((always_inline)) {
        constexpr int l = decltype(lc)::value;
        bool weak_l[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) weak_l[ct] = false;
        auto segment = [&](auto sc) __attribute__((always_inline)) {
        constexpr int sg = decltype(sc)::value;
        double best[CT], second[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) best[ct] = second[ct] = 1.0e300;
        // a group's bias and table rows are requested one group AHEAD of their use (the first group's under the tile's last MFMAs): a wave is
        // alone on its SIMD, so a load issued where it is used costs its whole L2 round trip (measured on the one-segment kernel)
        v4i qb[2][2], qt[2][l > 0 ? l * SEGS : 1][CT];
        auto issue = [&](int T, int g, int slot) __attribute__((always_inline)) {
            const int col = sg * a.kc + 32 * T + 8 * g;                 // the score inside the level: + 4 hf + e
            const int kofs = l * a.ke + col;
            qb[slot][0] = (v4i)__builtin_amdgcn_raw_buffer_load_b128(brs, 32 * hf, kofs * 8, 0);
            qb[slot][1] = (v4i)__builtin_amdgcn_raw_buffer_load_b128(brs, 32 * hf + 16, kofs * 8, 0);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
                for (int jj = 0; jj < l; ++jj)
#pragma unroll
                    for (int sp = 0; sp < SEGS; ++sp)
                        qt[slot][jj * SEGS + sp][ct] = (v4i)__builtin_amdgcn_raw_buffer_load_b128(trs, o[jj][sp][ct], ((l * (l - 1) / 2 + jj) * tsz + col) * 4, 0);
            }
        };
#pragma unroll 1
        for (int T = 0; T < ntile; ++T) {
            v16i acc[LIMBS][CT];
#pragma unroll
            for (int lb = 0; lb < LIMBS; ++lb)
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[lb][ct][r] = 0;
#pragma unroll
            for (int f = 0; f < LIMBS * 8; ++f) {
                const v4i A = ring[f % NPF];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[f >> 3][ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A, xb[ct][f & 7], acc[f >> 3][ct], 0, 0, 0);
                ring[f % NPF] = gload(f + NPF);
                if (f == LIMBS * 8 - 6) issue(T, 0, 0);
                __builtin_amdgcn_sched_barrier(0);                      // (hipcc otherwise sinks every load to its first use)
            }
            wo += LIMBS * 8 * 1024;
            // ---- the tile's 32 scores of each cell: lane (j, hf) holds scores 32 T + 8 g + 4 hf + e, g = r >> 2, e = r & 3 -----------------
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (g < 3) issue(T, g + 1, (g + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
                const int sl = g & 1;
                double b[4];                                            // 256 * bias + k: the packed form
                b[0] = __builtin_bit_cast(double, ((unsigned long long)(unsigned)qb[sl][0][1] << 32) | (unsigned)qb[sl][0][0]);
                b[1] = __builtin_bit_cast(double, ((unsigned long long)(unsigned)qb[sl][0][3] << 32) | (unsigned)qb[sl][0][2]);
                b[2] = __builtin_bit_cast(double, ((unsigned long long)(unsigned)qb[sl][1][1] << 32) | (unsigned)qb[sl][1][0]);
                b[3] = __builtin_bit_cast(double, ((unsigned long long)(unsigned)qb[sl][1][3] << 32) | (unsigned)qb[sl][1][2]);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int r = 4 * g + e;
                        // 256 S + k = 256 (65536 a2 + [256 a1 + a0 + tables] + bias) + k: the bracket in i32 (|a1| <= 2^22, |a0| <= 2^22,
                        // l * SEGS table entries below 2^29 / max(2, SEGS (levels - 1)): encode_two_stage.py refuses larger ones), the rest
                        // on integers below 2^52 in fp64 -- all exact
                        int lo = (acc[1][ct][r] << 8) + acc[0][ct][r];
#pragma unroll
                        for (int q = 0; q < l * SEGS; ++q) lo += qt[sl][q][ct][e];
                        double c = __builtin_fma((double)lo, 256.0, b[e]);
                        c = __builtin_fma((double)acc[2][ct][r], 16777216.0, c);
                        second[ct] = fmin(second[ct], fmax(best[ct], c));
                        best[ct] = fmin(best[ct], c);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // ---- close the segment: the two half-waves' (best, second), the index out of the packed value, the gap against the bound ------------
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const double ob = shfl_xor_f64(best[ct], 32), os = shfl_xor_f64(second[ct], 32);
            const double nb = fmin(best[ct], ob), ns = fmin(fmax(best[ct], ob), fmin(second[ct], os));
            const int c = (int)((long long)nb & 255);
            if (l < 2) o[l < 2 ? l : 0][sg][ct] = ((sg * a.kc + c) * a.ke + 4 * hf) * 4;
            const float t = ((a.tau[l][0] + a.tau[l][1] * n0[ct]) + (a.tau[l][2] * n0[ct]) * n0[ct]) + n1[ct];
            weak_l[ct] |= !(ns - nb > 256.0 * (double)ceilf(t) + 255.0);          // (not accepted: the gap in S is <= ceil(t))
            if (hf == 0 && m[ct] < a.M) a.codes[(size_t)(l * SEGS + sg) * a.M + m[ct]] = (uint8_t)c;
        }
        };
        segment(IC<0>{});
        if constexpr (SEGS > 1) segment(IC<1>{});
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
            if (weak_l[ct] && first[ct] == 3) first[ct] = l;           // a level is undecided if any of its segments is
    };
    level(IC<0>{});
    if (a.levels > 1) level(IC<1>{});
    if (a.levels > 2) level(IC<2>{});
    // ---- the cells stage 2 recomputes, in THREE lists by the level they are first undecided at (list c at a.list + c M, its length in
    //      counters[1 + c], counters[0] = all of them): a cell of list c has PROVEN codes below level c, so stage 2 skips the quantization
    //      head and the distances of those levels for it (codebook_encode_wave.hip).  No particular order inside a list. ------------------
    // (ONE returning atomic per list and wave, the three issued together: a returning atomic is a whole L2 round trip for a lone wave --
    //  the one-segment kernel measured one per list and cell tile at 15 % of its time)
    unsigned long long mask[3][CT];
    unsigned cnt[3] = {0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            mask[c][ct] = __builtin_amdgcn_ballot_w64(first[ct] == c && hf == 0 && m[ct] < a.M);
            cnt[c] += (unsigned)__builtin_popcountll(mask[c][ct]);
        }
    // ... and one per list and WORKGROUP: the waves' counts meet in LDS, wave 0 reserves the workgroup's ranges
    __shared__ unsigned wcnt[4][3], wbase[3];
    if (lane == 0) { wcnt[wave][0] = cnt[0]; wcnt[wave][1] = cnt[1]; wcnt[wave][2] = cnt[2]; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned tot = wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
        wbase[threadIdx.x] = tot ? atomicAdd(a.counters + 1 + threadIdx.x, tot) : 0u;
        if (tot) atomicAdd(a.counters, tot);
    }
    __syncthreads();
    unsigned base[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        base[c] = wbase[c];
        for (int w2 = 0; w2 < wave; ++w2) base[c] += wcnt[w2][c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        unsigned at = __builtin_amdgcn_readfirstlane(base[c]);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            if (first[ct] == c && hf == 0 && m[ct] < a.M)
                a.list[(size_t)c * a.M + at + (unsigned)__builtin_popcountll(mask[c][ct] & ((1ull << lane) - 1ull))] = (unsigned)m[ct];
            at += (unsigned)__builtin_popcountll(mask[c][ct]);
        }
    }
}

__global__ void zero_seg_counters_kernel(unsigned* c) { if (threadIdx.x < 4) c[threadIdx.x] = 0; }

}  // namespace
}  // namespace qv2x

extern "C" int qv2x_codebook_encode_candidates_seg_i8(const qv2x_encode_desc* d, const int8_t* in, const int8_t* g_limbs, const double* bias_packed,
                                                      const int32_t* tables, const float* tau, uint8_t* codes, uint32_t* list, uint32_t* counters,
                                                      void* stream) {
    using namespace qv2x;
    const char* me = "qv2x_codebook_encode_candidates_seg_i8";
    if (!d || !in || !g_limbs || !bias_packed || !tau || !codes || !list || !counters) return fail(QV2X_EINVAL, "%s: null pointer", me);
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->levels < 1 || d->levels > 3) return fail(QV2X_EINVAL, "%s: 1..3 levels", me);
    const int segs = d->segs ? d->segs : 1;
    if (segs != 1 && segs != 2) return fail(QV2X_EINVAL, "%s: seg_num 1 or 2 (got %d; the exact entry takes 4)", me, d->segs);
    // (seg_num <= 2 and dict_size <= 256 together are the header's seg_num * dict_size <= 512: no check of its own)
    if (d->kc < 32 || d->kc > 256 || d->kc % 32 || (segs > 1 && d->kc % 64))
        return fail(QV2X_EINVAL, "%s: dict_size a multiple of 32 up to 256 (of 64 with two segments; got %d x %d)", me, segs, d->kc);
    if (d->levels > 1 && !tables) return fail(QV2X_EINVAL, "%s: the residual levels need their tables", me);
    if (d->in_zx < 0 || d->in_zx > 255) return fail(QV2X_EINVAL, "%s: in_zx outside 0..255", me);
    if (((uintptr_t)in & 15) || ((uintptr_t)g_limbs & 15) || ((uintptr_t)tables & 15) || ((uintptr_t)bias_packed & 7))
        return fail(QV2X_EALIGN, "%s: 16-byte aligned maps, limbs and tables", me);
    CandSegArgs a;
    a.in = in; a.gpack = g_limbs; a.bias = bias_packed; a.tables = tables; a.codes = codes; a.list = list; a.counters = counters;
    for (int l = 0; l < 3; ++l)
        for (int i = 0; i < 3; ++i) a.tau[l][i] = l < d->levels ? tau[l * 3 + i] : 0.0f;
    a.n = d->n; a.h = d->h; a.w = d->w; a.hw = d->h * d->w; a.M = d->n * a.hw; a.levels = d->levels; a.kc = d->kc; a.ke = segs * d->kc; a.zx = d->in_zx;
    a.gbytes = d->levels * (a.ke / 32) * LIMBS * 8 * 1024;
    a.tbytes = (d->levels > 1 ? d->levels * (d->levels - 1) / 2 : 1) * a.ke * a.ke * 4;
    a.delta = d->in_delta;
    hipStream_t st = (hipStream_t)stream;
    zero_seg_counters_kernel<<<1, 64, 0, st>>>(counters);
    int dev = 0, cus = 256, v = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
    // the large tile from two rounds of the chip's SIMDs on (as the one-segment kernel switches), the 64-cell wave below
    const int big = segs == 2 ? QV2X_CAND_SEG_CT2 : QV2X_CAND_SEG_CT1;
    const bool large = a.M >= 4 * cus * 32 * big * 2;
    auto grid = [&](int ct) { return (unsigned)((a.M + 128 * ct - 1) / (128 * ct)); };
    if (segs == 2) {
        if (large) encode_candidates_seg_kernel<QV2X_CAND_SEG_CT2, 2><<<grid(QV2X_CAND_SEG_CT2), 256, 0, st>>>(a);
        else encode_candidates_seg_kernel<2, 2><<<grid(2), 256, 0, st>>>(a);
    } else {
        if (large) encode_candidates_seg_kernel<QV2X_CAND_SEG_CT1, 1><<<grid(QV2X_CAND_SEG_CT1), 256, 0, st>>>(a);
        else encode_candidates_seg_kernel<2, 1><<<grid(2), 256, 0, st>>>(a);
    }
    return hip_check(hipGetLastError(), "qv2x_codebook_encode_candidates_seg_i8 launch");
}
