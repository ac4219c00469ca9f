// Argument pack of the BatchNorm backward that the act16 attention backward
// applies in its row kernel's prologue (launch_edge_attn_fused_bwd16).  Plain
// types only: the binding layer fills it, the launcher reads it.
#pragma once

struct AttnBnBwd {
  const void* x;              // bf16 [n, h]: BN input (the attention output)
  const unsigned char* mask;  // [n, h/8] keep mask of the BN forward
  const float* mean;          // [h]
  const float* invstd;        // [h]
  const float* gamma;         // [h]
  const float* partials;      // [2h]: per-channel sums of gm and gm*xhat
  const float* count_ptr;     // device-side global row count, or null
  long count;                 // row count used when count_ptr is null
  float keep_inv;             // 1/(1-p) of the fused dropout, 1 without
};

// Argument pack of the pattern-pool backward that the last conv's attention
// backward forms itself: the gradient of node i is gout[batch[i]] * probs[i] /
// nn[i] (pool_bwd_dx in common.h), so neither kernel reads an [n, h] gradient.
// A null gout means off.
struct AttnPoolBwd {
  const float* gout;   // [graphs, h]: gradient of the pooled output
  const float* probs;  // [n]
  const float* nn;     // [n]
  const long* batch;   // [n]: graph of each node
};
