// The plan of an LPIPS training call, shared by the forward that keeps what the backward needs (lpips.hip,
// grpg_lpips_forward_train) and the backward (lpips_bwd.hip, grpg_lpips_backward): where every layer's output, the
// per-pixel maps, the slots and the backward's gradient buffers lie in the training workspace.
#pragma once
#include <cstddef>

namespace grpg {

constexpr int LPT_TAPS = 5;
constexpr int LPT_MAX_LAYERS = 17;   // VGG16 up to its fifth tap: 13 convolutions + 4 pools

struct LpipsTrainLayer {
  int pool;                 // 0: convolution + ReLU, 1: max-pool
  int c_in, c_out, k, stride, pad;
  int tap;                  // the tap this layer's output is, or -1
  int h_in, w_in, h_out, w_out;
  size_t out_off;           // bytes from the workspace's start: [2 * pairs, c_out, h_out, w_out], x's images first.
                            // A convolution's output is kept; the pools share ONE buffer (a pool's output is read
                            // by the next convolution only, and never by the backward)
};

struct LpipsTrainPlan {
  int n_layers, n_convs;
  LpipsTrainLayer L[LPT_MAX_LAYERS];
  int tap_c[LPT_TAPS], tap_hw[LPT_TAPS], tap_nblk[LPT_TAPS];
  size_t map_off[LPT_TAPS], slot_off[LPT_TAPS];
  size_t grad_off[2];       // the backward's two ping-pong gradients: the largest [pairs, c_out, h_out, w_out]
  size_t tapgrad_off;       // one tap's gradient: the largest [pairs, C_l, H_l, W_l]
  size_t total;
};

// false: a size the entry points refuse (exactly those grpg_lpips_workspace_bytes refuses)
bool lpips_train_plan(int net, int pairs, int h, int w, LpipsTrainPlan& P);

}  // namespace grpg
