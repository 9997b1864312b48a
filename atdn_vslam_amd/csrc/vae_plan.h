// Geometry of the MappingVAE encoder (vae.hip) for one frame size: what every stage writes and how many floats per image each
// of the four scratch buffers has to hold. Host only (no HIP here): finalize() allocates from it, encode() checks every launch
// against it, and atdn_vae_scratch_floats exports it so that a test without a GPU can restate it.
#pragma once

namespace atdn {

constexpr int kVaeStages = 7;                                        // stage 0 = the 7x7 stem, 1..6 = the residual blocks
constexpr int kVaeChannels[kVaeStages] = {3, 16, 16, 32, 64, 128, 128};  // channels each stage writes

// channels per pixel of a stored map: ROW-mode layers read 4 or 16 dense channels, TAP-mode layers multiples of 32
inline int vae_pix_channels(int c) { return c <= 4 ? 4 : c <= 16 ? 16 : (c + 31) / 32 * 32; }

struct VaePlan {
  int h[kVaeStages], w[kVaeStages], ld[kVaeStages];  // output of stage k as the next layer reads it: h x w pixels of ld floats
  long in4, bufA, bufB, bufS;                        // floats per image
};

// H, W >= 1. Every residual block is conv.0 (3x3, stride 1: the block's input size and channels, into bufB), the skip convolution
// (1x1, stride 2, no padding, into bufS) and conv.1 (3x3, stride 2, padding 1, into bufA, which also holds the stem's output):
// both stride-2 layers write ceil(h/2) x ceil(w/2) pixels, which is more than h*w/4 as soon as h or w is odd.
inline VaePlan vae_plan(int H, int W) {
  VaePlan p{};
  auto grow = [](long& cap, long n) { if (n > cap) cap = n; };
  p.h[0] = H; p.w[0] = W; p.ld[0] = vae_pix_channels(kVaeChannels[0]);   // 7x7, stride 1, padding 3
  p.in4 = (long)H * W * 4;
  grow(p.bufA, (long)H * W * p.ld[0]);
  for (int k = 1; k < kVaeStages; ++k) {
    grow(p.bufB, (long)p.h[k - 1] * p.w[k - 1] * p.ld[k - 1]);
    p.h[k] = (p.h[k - 1] - 1) / 2 + 1; p.w[k] = (p.w[k - 1] - 1) / 2 + 1; p.ld[k] = vae_pix_channels(kVaeChannels[k]);
    const long out = (long)p.h[k] * p.w[k] * p.ld[k];
    grow(p.bufS, out);
    grow(p.bufA, out);
  }
  return p;
}

}  // namespace atdn
