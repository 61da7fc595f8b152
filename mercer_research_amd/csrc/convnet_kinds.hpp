// convnet_kinds.hpp -- Track X host: the ONE table of layer kinds (rcn_hipx_layer_kind, include/rcn_hipx.h).  Host only, no device code.
// A row says what the walks of rcn_hipx_api.hip (describe_layers, forward, backward_layers, the state and statistics entry points) ask of a
// kind.  A new kind is declared by one row here, one arm in each of the three dispatch functions beside the launchers (layer_forward,
// layer_dgrad, layer_wgrad) and its shape rules in describe_layers.  A kind's name in a message comes from its row.
#pragma once
#include "../../include/rcn_hipx.h"

namespace rcnx {

struct KindRow {
    const char* name;       // the ABI name
    int ks, stride;         // filter size of a [W | b] block (3: the 3x3 convolutions, the depthwise one too, K = 9 = 3 x 3 x 1; else 1), and stride
    bool map;               // a convolution: a matrix layer whose rows are the pixels of a map, not the samples of a batch (a dense layer)
    bool gemm;              // a GEMM layer: bf16 operand copies (prep_bf16_weights); the depthwise convolution computes in fp32 in either mode
    bool linear;            // bias only, no activation and no ReLU gate of its own: batch normalisation must follow directly
    bool bn;                // batch normalisation, with or without a skip: a [gamma | beta] block (K = 1), statistics and buffers
    bool params;            // a parameter block, [W | b] or [gamma | beta]: every kind but the two pools, which also take no `out`
    bool matrix;            // ... whose W is a matrix with a tap-flipped transposed copy: every block but batch normalisation's
    bool relu;              // a ReLU of its own on its output (bn && !relu: RCN_HIPX_BN, RCN_HIPX_BN_ADD -- never gated, and a convolution must follow)
    bool named;             // its refusals name the layer, "layer i (KIND): ": the kinds from RCN_HIPX_GLOBAL_AVGPOOL on and the two skip kinds
};

constexpr KindRow kKinds[] = {
    // (indexed by kind)        ks st  map gemm lin bn par mat relu named
    {"RCN_HIPX_CONV3X3_RELU",     3, 1,  1,  1,  0,  0,  1,  1,  1,  0},      // 0
    {"RCN_HIPX_MAXPOOL2",         1, 2,  0,  0,  0,  0,  0,  0,  0,  0},      // 1
    {"RCN_HIPX_DENSE_RELU",       1, 1,  0,  1,  0,  0,  1,  1,  1,  0},      // 2
    {"RCN_HIPX_DENSE",            1, 1,  0,  1,  0,  0,  1,  1,  0,  0},      // 3
    {"RCN_HIPX_CONV3X3",          3, 1,  1,  1,  1,  0,  1,  1,  0,  0},      // 4
    {"RCN_HIPX_BN_RELU",          1, 1,  0,  0,  0,  1,  1,  0,  1,  0},      // 5
    {"RCN_HIPX_BN_ADD_RELU",      1, 1,  0,  0,  0,  1,  1,  0,  1,  1},      // 6
    {"RCN_HIPX_GLOBAL_AVGPOOL",   1, 1,  0,  0,  0,  0,  0,  0,  0,  1},      // 7
    {"RCN_HIPX_CONV3X3_S2",       3, 2,  1,  1,  1,  0,  1,  1,  0,  1},      // 8
    {"RCN_HIPX_BN_ADD_RELU_DOWN", 1, 1,  0,  0,  0,  1,  1,  0,  1,  1},      // 9
    {"RCN_HIPX_CONV1X1",          1, 1,  1,  1,  1,  0,  1,  1,  0,  1},      // 10
    {"RCN_HIPX_DWCONV3X3",        3, 1,  1,  0,  1,  0,  1,  1,  0,  1},      // 11
    {"RCN_HIPX_BN",               1, 1,  0,  0,  0,  1,  1,  0,  0,  1},      // 12
    {"RCN_HIPX_BN_ADD",           1, 1,  0,  0,  0,  1,  1,  0,  0,  1},      // 13
    {"RCN_HIPX_DWCONV3X3_S2",     3, 2,  1,  0,  1,  0,  1,  1,  0,  1},      // 14
};
constexpr int kKindCount = RCN_HIPX_DWCONV3X3_S2 + 1;         // (the enum's last value: a new kind moves it)
static_assert(sizeof(kKinds) / sizeof(kKinds[0]) == kKindCount, "one row per rcn_hipx_layer_kind");

// the row of a kind; a value that is no kind (describe_layers refuses it) reads as a layer that is nothing
constexpr KindRow kNoKind{"unknown", 1, 1, 0, 0, 0, 0, 0, 0, 0, 0};
inline const KindRow& kind_row(int kind) { return kind >= 0 && kind < kKindCount ? kKinds[kind] : kNoKind; }

}  // namespace rcnx
