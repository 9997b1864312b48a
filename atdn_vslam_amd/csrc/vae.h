// MappingVAE encoder (atdn_vslam/localization/network.py:29-45,57-70): the embedding `mu` that NeuralSLAM's
// relocalisation compares between a query frame and the stored keyframes. Decoder and training stay outside.
#pragma once
#include "conv_dispatch.h"
#include "device_buf.h"
#include "kernels.h"
#include "weights.h"
#include "vae_plan.h"

namespace atdn {

class VaeEncoder {
 public:
  VaeEncoder(int H, int W, int max_batch);
  StateDict& state() { return sd_; }
  void finalize();
  // images NCHW [B,3,H,W] with values 0..255 -> mu NHWC [B][h*w][128] (h, w = out_h(), out_w())
  void encode(const float* images, int B, float* mu, hipStream_t st);
  // tests only: runs the stack up to stage k (0 = stem, 1..6 = residual blocks) and copies its output, as the next layer reads
  // it, to `out` (device, `capacity` floats): NHWC [B][plan().h[k]][plan().w[k]][plan().ld[k]], pad lanes included
  void debug_stage(const float* images, int B, int k, float* out, long capacity, hipStream_t st);
  const VaePlan& plan() const { return plan_; }
  int out_h() const { return oh_; }
  int out_w() const { return ow_; }

  int H, W, maxB;

 private:
  struct ConvBN { PackedConv conv; long sc_off = -1, sh_off = -1; const float* sc = nullptr; const float* sh = nullptr; };
  struct Res { ConvBN a, b; PackedConv skip; long sc_off = -1, sh_off = -1; const float* sc = nullptr; const float* sh = nullptr; };
  ConvBN pack_convbn(const std::string& p);
  void run(const float* images, int B, int last_stage, float* mu, hipStream_t st);

  StateDict sd_;
  WeightArena arena_;
  bool ready_ = false;
  ConvBN stem_;
  Res res_[6];
  PackedConv mean_;
  DeviceBuf in4_, bufA_, bufB_, bufS_;
  VaePlan plan_;
  int oh_ = 0, ow_ = 0;
};

}  // namespace atdn
