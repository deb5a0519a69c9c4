// qv2x_conv3x3_i8_wide and its weights-stationary forms (conv_i8_wide.hip, conv_i8_ws.hip, conv_i8_ws2.hip): what passes between them.
#pragma once
#include "conv_host.h"

namespace qv2x {

// what fill_args fills and the wide kernels take (there as the file-local WideArgs, which adds nothing: a kernel's symbol carries its
// argument type's name); field order and layout are the kernels' kernarg loads
constexpr int MAX_CHUNKS = 24;
struct WideFields {
    const int8_t* in; const int8_t* wt; const float* scale; const int* corr; const int* aw; const float* bias; int8_t* out;
    int n, hp, wp, cin_total, cout, ho, wo, tiles_x, tiles_y;
    int out_ctotal, out_c0, relu;
    float out_delta, out_zp;
    int nchunks, ngroups;
    int wtile;                        // rows of one pre-tiled weight tile: min(cout, 256)
    int cend[QV2X_MAX_GROUPS];        // first chunk index past group g
    int coff[MAX_CHUNKS];        // channel byte offset of each 64-channel chunk inside a pixel
    int items;                        // (patch, channel block) pairs, patches padded to a multiple of 8
    int nsteps;                       // weight steps of an item's K loop: 9 per 64 input channels
    int stride2;                      // 1: the stride-2 form (four parity-plane chunks per 64 input channels)
};
// the weights-stationary forms of qv2x_conv3x3_i8_wide for 64 input channels (same w_wide layout, same results; `w` filled and checked there)
bool ws64_takes(const qv2x_conv_desc* d);                              // conv_i8_ws.hip: stride 1, 64 -> 64
bool ws2_takes(const qv2x_conv_desc* d);                               // conv_i8_ws2.hip: stride 2, 64 -> 64 | 128
int launch_ws64(const WideFields& w, hipStream_t st);
int launch_ws2(const WideFields& w, hipStream_t st);
// the fields WsArgs and Ws2Args share with it; their patches are `th` x 32 outputs (the wide kernel's own: 5 x 32, the same tiles_x)
template <class A> void ws_args(A& a, const WideFields& w, int th) {
    a.in = w.in; a.wt = w.wt; a.scale = w.scale; a.corr = w.corr; a.aw = w.aw; a.bias = w.bias; a.out = w.out;
    a.n = w.n; a.hp = w.hp; a.wp = w.wp; a.cin_total = w.cin_total; a.cin_off = w.coff[0]; a.cout = w.cout;
    a.ho = w.ho; a.wo = w.wo; a.tiles_x = w.tiles_x; a.tiles_y = tiles(w.ho, th);
    a.out_ctotal = w.out_ctotal; a.out_c0 = w.out_c0; a.relu = w.relu; a.out_delta = w.out_delta; a.out_zp = w.out_zp;
    a.items = a.n * a.tiles_x * a.tiles_y;
}

}  // namespace qv2x
