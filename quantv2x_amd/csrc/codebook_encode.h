// Shared by the two forms of a6 (codebook_encode.hip: a workgroup per 32 / 64 cells; codebook_encode_wave.hip: a wave per 32 cells).
#pragma once
#include "common.h"

namespace qv2x {

constexpr int ENC_D = 256;
constexpr int ENC_WAVE_PAD = 16 * 256;      // floats behind the wave-form section: its weight ring reads 16 groups (1 KiB each) ahead

struct EncArgs {
    const int8_t* in; const float* in_f32; uint8_t* codes;      // in_f32 != null: the rows come as fp32 (un-quantized model)
    const float* lvl[4];
    int n, h, w, levels, kc, ax, M;     // kc: codes per SEGMENT and level
    int segs, ke;                       // seg_num (m) = 1 | 2 | 4 segments of 256 / segs dims; ke = segs * kc rows of the extended codebook
    float dx;
    int m_lo, m_hi;             // the rows [m_lo, m_hi) of the M = n h w cells this launch encodes (a launch may be split between the two forms)
    int list_slots = 1, list_tail_max = 0;                 // the split of the listed cells between the two forms (codebook_encode.hip:list_full_tiles)
    const unsigned* list = nullptr; const unsigned* list_count = nullptr;      // LIST forms: the cells to encode (three lists) and their DEVICE-side counts (list_plan below)
};

// A level blob (include/qv2x.h): the workgroup form's section, then the wave form's.  `kc` here = rows of the (extended) codebook.
__device__ __host__ __forceinline__ int64_t level_floats_wg(int kc) { return 3LL * (ENC_D * ENC_D + ENC_D) + (int64_t)ENC_D * kc + (int64_t)kc * ENC_D + kc; }
__device__ __host__ __forceinline__ int64_t level_floats(int kc) { return level_floats_wg(kc) + 3LL * ENC_D * ENC_D + (int64_t)((kc + 63) / 64 * 64) * ENC_D + ENC_WAVE_PAD; }

// ---- stage 2 of the two-stage encode: the listed cells (codebook_encode_cand.hip writes them) --------------------------------------------------
// THREE lists by the level a cell is first undecided at: list c at a.list + c * a.M, its length at a.list_count[1 + c] (a.list_count[0] = all of
// them).  Tiles of 32 cells are numbered list by list; whole rounds of the wave form's `list_slots` persistent waves take tiles [0, full), the
// workgroup form the rest (up to `list_tail_max` tiles; a larger remainder is one more round of waves).  Both kernels derive the same plan from
// the DEVICE-side counts.
struct ListPlan { int n[3], first[3], total, full; };
__device__ __forceinline__ ListPlan list_plan(const EncArgs& a) {
    ListPlan p;
    int t = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) { p.n[c] = (int)a.list_count[1 + c]; p.first[c] = t; t += (p.n[c] + 31) >> 5; }
    p.total = t;
    const int full = t / a.list_slots * a.list_slots;
    p.full = t - full > a.list_tail_max ? t : full;
    return p;
}
// tile -> (list, first entry of the tile inside it)
__device__ __forceinline__ void list_tile(const ListPlan& p, int tile, int& cls, int& i0) {
    cls = tile >= p.first[2] ? 2 : (tile >= p.first[1] ? 1 : 0);
    i0 = (tile - p.first[cls]) * 32;
}

// ---- the span form of stage 2 (qv2x_codebook_encode_span_f32; codebook_encode_cand.hip's span entry writes its lists) -----------------------
// SIX lists by the (first, last) undecided level of a cell, dearest first by the work stage 2 spends on the class -- 2 f products of latent
// chain in front, 2.5 per level f .. l (stage, qhead, distances), 1 per lhead in between:
//     class   0       1       2       3       4       5
//     (f, l)  (0, 2)  (1, 2)  (2, 2)  (0, 1)  (1, 1)  (0, 0)
//     cost    9.5     8       6.5     6       4.5     2.5
// List k at a.list + k * a.M, its length at a.list_count[1 + k] (a.list_count[0] = all of them).  The listed cells are ONE sequence -- list 0,
// then list 1, ... -- cut into tiles of 32, so only a tile on a class boundary holds cells of two classes and only the last tile is partial.
// Whole rounds / remainder: the rule of list_plan.
constexpr int SPAN_CLASSES = 6;
__device__ __host__ __forceinline__ constexpr int span_first(int k) { return k < 3 ? k : (k < 5 ? k - 3 : 0); }
__device__ __host__ __forceinline__ constexpr int span_last(int k) { return k < 3 ? 2 : (k < 5 ? 1 : 0); }
// (first, last) -> class; last >= first
__device__ __host__ __forceinline__ constexpr int span_class(int first, int last) { return last == 2 ? first : (last == 1 ? 3 + first : 5); }
struct SpanPlan { int pre[SPAN_CLASSES + 1], total, full; };          // pre[k]: listed cells in front of list k; total / full in tiles
__device__ __forceinline__ SpanPlan span_plan(const EncArgs& a) {
    SpanPlan p;
    p.pre[0] = 0;
#pragma unroll
    for (int k = 0; k < SPAN_CLASSES; ++k) p.pre[k + 1] = p.pre[k] + (int)a.list_count[1 + k];
    p.total = (p.pre[SPAN_CLASSES] + 31) >> 5;
    const int full = p.total / a.list_slots * a.list_slots;
    p.full = p.total - full > a.list_tail_max ? p.total : full;
    return p;
}
// entry i of the sequence (clamped to the last one: a partial tile's idle lanes repeat it) -> the cell and its class
__device__ __forceinline__ int span_cell(const SpanPlan& p, const EncArgs& a, int i, int& cls) {
    i = i < p.pre[SPAN_CLASSES] ? i : p.pre[SPAN_CLASSES] - 1;
    int base = 0;
    cls = 0;
#pragma unroll
    for (int k = 1; k < SPAN_CLASSES; ++k)
        if (i >= p.pre[k]) { cls = k; base = p.pre[k]; }
    return (int)a.list[(size_t)cls * a.M + (i - base)];
}

// codebook_encode_wave.hip
int encode_wave_launch(const EncArgs& a, hipStream_t st);      // rows [a.m_lo, a.m_hi): one wave per 32
// the cells a.list[0 .. *a.list_count): persistent waves; `span`: the six span lists, a tile ends at its last undecided level
int encode_wave_list_launch(const EncArgs& a, int waves, bool span, hipStream_t st);

// codebook_encode.hip.  The descriptor rules every entry of the encode family shares (the 64-wide, candidate and collapsed entries too), in the
// messages of the entry `me`: `d` and the entry's other pointers (`ptrs`: all of them there) not null; n, h, w positive; 1 .. max_levels levels;
// seg_num 1 | 2 | 4 up to max_segs (0 = 1: a descriptor from before the field existed); dict_size a multiple of 32 (of 64 with more than one
// segment) up to max_kc, seg_num * dict_size <= 512 (sixteen 32-code tiles of the extended codebook).
// Returns the effective seg_num, or the error (QV2X_EINVAL) after fail().
int encode_check(const char* me, const qv2x_encode_desc* d, bool ptrs, int max_levels, int max_segs, int max_kc);

}  // namespace qv2x
