// Host side of the int8 convolution family (conv_i8*.hip, conv1x1_i8.hip, gconv3x3_i8.hip, bottleneck_i8.hip): the sizes every entry derives
// from its descriptor and the one statement of the qv2x_conv_desc group rule.
#pragma once
#include "common.h"

namespace qv2x {

// outputs per axis of a padded 3x3 layer -- (in + 2 - 3) / stride + 1 -- and of a strided 1x1 layer: the same number
constexpr int conv_out(int in, int stride) { return (in - 1) / stride + 1; }
constexpr int tiles(int x, int t) { return (x + t - 1) / t; }

// One walk over a descriptor's input groups (ngroups already checked): a group is c > 0 channels, a multiple of 64, from a multiple of 16,
// inside cin_total.  `bad` = the first group that is not (-1: none), `chunks` = the 64-channel chunks of the groups in front of it.
struct GroupWalk { int bad, chunks; };
inline GroupWalk walk_groups(const qv2x_conv_desc* d) {
    GroupWalk w{-1, 0};
    for (int g = 0; g < d->ngroups && w.bad < 0; ++g) {
        const int c0 = d->group_c0[g], c = d->group_c[g];
        if (c <= 0 || c % 64 || c0 % 16 || c0 + c > d->cin_total) w.bad = g;
        else w.chunks += c / 64;
    }
    return w;
}
#define QV2X_GROUP_RULE "group %d (c0=%d, c=%d): channels must come in multiples of 64"      // a bad group's message, after the entry's name

}  // namespace qv2x
