// MappingVAE encoder on MI355X. Reference: atdn_vslam/localization/network.py:29-45 (layers), 57-70 (forward,
// non-variational: mu = mean_lin(encoder(normalize(image)))); layers/conv.py:36-37 (Conv = BN(Mish(conv))),
// 83-90 (ResidualConv); utils/normalizations.py:4-6 (x/255, then ImageNet mean/std).
#include "vae.h"

namespace atdn {

extern template TileChoice conv_dispatch<MODE_ROW, EpiBias<ACT_NONE>>(const ConvShape&, EpiBias<ACT_NONE>, hipStream_t);
extern template TileChoice conv_dispatch<MODE_ROW, EpiMishBN>(const ConvShape&, EpiMishBN, hipStream_t);
extern template TileChoice conv_dispatch<MODE_ROW, EpiMishBNSkipMishBN>(const ConvShape&, EpiMishBNSkipMishBN, hipStream_t);
extern template TileChoice conv_dispatch<MODE_TAP, EpiBias<ACT_NONE>>(const ConvShape&, EpiBias<ACT_NONE>, hipStream_t);
extern template TileChoice conv_dispatch<MODE_TAP, EpiMishBN>(const ConvShape&, EpiMishBN, hipStream_t);
extern template TileChoice conv_dispatch<MODE_TAP, EpiMishBNSkipMishBN>(const ConvShape&, EpiMishBNSkipMishBN, hipStream_t);

namespace {
inline int conv_mode(int cin) { return cin >= 32 ? MODE_TAP : MODE_ROW; }

template <class Epi>
void run_conv(int mode, const ConvShape& s, const Epi& ep, hipStream_t st) {
  if (mode == MODE_TAP) conv_dispatch<MODE_TAP>(s, ep, st);
  else conv_dispatch<MODE_ROW>(s, ep, st);
}
}  // namespace

VaeEncoder::VaeEncoder(int H_, int W_, int max_batch) : H(H_), W(W_), maxB(max_batch) {
  ATDN_CHECK(max_batch >= 1 && max_batch <= 64, "max_batch out of range");
  ATDN_CHECK(H >= 64 && W >= 64 && (long)H * W <= (1L << 24), "frame size out of range");
  plan_ = vae_plan(H, W);
  oh_ = plan_.h[kVaeStages - 1]; ow_ = plan_.w[kVaeStages - 1];
}

VaeEncoder::ConvBN VaeEncoder::pack_convbn(const std::string& p) {
  ConvBN c;
  const HostTensor& w = sd_.get(p + ".conv.weight");
  const int cout = (int)w.shape[0], cin = (int)w.shape[1];
  const int mode = conv_mode(cin);
  const int ldo = vae_pix_channels(cout);
  // A layer that computes fewer channels than its map carries per pixel (3 of 4: the stem and conv.0 of the first block) gets
  // the missing output channels as rows of zeros: weight, bias, scale and shift 0. The kernel then writes the pad lane itself, 0
  // on every finite frame, so the next layer never reads what an earlier call left there. The pad lane meets zero weights,
  // but 0 * NaN is NaN: a lane zeroed once at finalize() and later overwritten by the wider maps of a non-finite frame
  // would poison every later call on the handle.
  StateDict padded;
  if (ldo > cout) {
    const long per = w.numel() / cout;
    std::vector<float> wp((size_t)ldo * per, 0.f), bp((size_t)ldo, 0.f);
    std::copy(w.data.begin(), w.data.end(), wp.begin());
    const HostTensor& b = sd_.get(p + ".conv.bias");
    std::copy(b.data.begin(), b.data.end(), bp.begin());
    const int64_t ws[4] = {ldo, cin, w.shape[2], w.shape[3]}, bs[1] = {ldo};
    padded.put("padded.weight", wp.data(), ws, 4);
    padded.put("padded.bias", bp.data(), bs, 1);
  }
  c.conv = pack_conv(arena_, ldo > cout ? padded : sd_, {ldo > cout ? std::string("padded") : p + ".conv"}, mode,
                     mode == MODE_ROW ? vae_pix_channels(cin) : 0);
  ChannelAffine a = bn_affine(sd_, p + ".bn");
  std::vector<float> sc(a.scale.begin(), a.scale.end()), sh(a.shift.begin(), a.shift.end());
  sc.resize((size_t)ldo, 0.f); sh.resize((size_t)ldo, 0.f);
  c.sc_off = pack_vector(arena_, sc);
  c.sh_off = pack_vector(arena_, sh);
  return c;
}

void VaeEncoder::finalize() {
  ATDN_CHECK(!ready_, "finalize called twice");
  stem_ = pack_convbn("encoder.0");
  for (int i = 0; i < 6; ++i) {
    const std::string p = "encoder." + std::to_string(i + 1);
    const int cin = kVaeChannels[i];
    ATDN_CHECK((int)sd_.get(p + ".conv.1.conv.weight").shape[0] == kVaeChannels[i + 1], "unexpected MappingVAE channel plan");
    res_[i].a = pack_convbn(p + ".conv.0");
    res_[i].b = pack_convbn(p + ".conv.1");
    const int mode = conv_mode(cin);
    res_[i].skip = pack_conv(arena_, sd_, {p + ".skip_layer"}, mode, mode == MODE_ROW ? vae_pix_channels(cin) : 0);
    ChannelAffine a = bn_affine(sd_, p + ".out_block.1");
    std::vector<float> sc(a.scale.begin(), a.scale.end()), sh(a.shift.begin(), a.shift.end());
    res_[i].sc_off = pack_vector(arena_, sc);
    res_[i].sh_off = pack_vector(arena_, sh);
  }
  mean_ = pack_conv(arena_, sd_, {"mean_lin"}, MODE_TAP, 0);
  arena_.upload();
  auto fix = [&](ConvBN& c) { resolve(arena_, c.conv); c.sc = arena_.dev(c.sc_off); c.sh = arena_.dev(c.sh_off); };
  fix(stem_);
  for (auto& r : res_) { fix(r.a); fix(r.b); resolve(arena_, r.skip); r.sc = arena_.dev(r.sc_off); r.sh = arena_.dev(r.sh_off); }
  resolve(arena_, mean_);
  // The stride-2 layers write ceil(h/2) x ceil(w/2) pixels, so H*W*4 floats per image hold every map only when H and W are even
  // (65 x 65: the first block writes 33*33*16 = 17424 floats, 4*65*65 = 16900); vae_plan() takes the largest map each buffer holds.
  // Nothing is cleared: every layer writes all the channels per pixel that the next one reads, and encode() reads only what the
  // same call has written.
  in4_.alloc(maxB * plan_.in4);
  bufA_.alloc(maxB * plan_.bufA);
  bufB_.alloc(maxB * plan_.bufB);
  bufS_.alloc(maxB * plan_.bufS);
  ready_ = true;
}

void VaeEncoder::encode(const float* images, int B, float* mu, hipStream_t st) { run(images, B, kVaeStages - 1, mu, st); }

void VaeEncoder::debug_stage(const float* images, int B, int k, float* out, long capacity, hipStream_t st) {
  ATDN_CHECK(k >= 0 && k < kVaeStages, "stage out of range");
  const long n = (long)B * plan_.h[k] * plan_.w[k] * plan_.ld[k];
  ATDN_CHECK(B >= 1 && capacity >= n, "output buffer too small for this stage");
  run(images, B, k, nullptr, st);
  ATDN_HIP(hipMemcpyAsync(out, bufA_.p, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));  // every stage ends in bufA_
}

// the stem and the residual blocks 1..last_stage; with `mu`, mean_lin on the last block's output
void VaeEncoder::run(const float* images, int B, int last_stage, float* mu, hipStream_t st) {
  ATDN_CHECK(ready_, "weights not finalized");
  ATDN_CHECK(B >= 1 && B <= maxB, "batch exceeds max_batch of this handle");
  // what a launch is about to write must fit its destination: B images of h x w pixels of ld floats
  auto fits = [&](const DeviceBuf& b, int h, int w, int ld) { return (long)B * h * w * ld <= b.n; };
  ATDN_CHECK(fits(in4_, H, W, 4), "MappingVAE scratch buffer too small for the normalised frames");
  launch_prep_rgb(images, B, H, W, in4_.p, st);
  auto shape = [&](const PackedConv& L, const float* src, int h, int w, int stride, int pad) {
    ConvShape s;
    s.src0 = src; s.ld0 = L.C; s.sb0 = (long)h * w * L.C; s.C0 = L.C; s.H = h; s.W = w;
    s.KH = L.KH; s.KW = L.KW; s.stride = stride; s.padH = pad; s.padW = pad;
    s.w = L.w; s.ldw = L.ldw; s.N = L.N; s.nimg = B;
    return s;
  };
  int h = H, w = W;
  float* x = bufA_.p; float* t = bufB_.p;
  int ldx = 4;  // channels per pixel of x as the next layer reads it
  ATDN_CHECK(stem_.conv.N == ldx && ldx == plan_.ld[0], "channel layout mismatch between VAE layers");
  ATDN_CHECK(fits(bufA_, h, w, ldx), "MappingVAE scratch buffer too small for the stem's output");
  run_conv(MODE_ROW, shape(stem_.conv, in4_.p, h, w, 1, 3),
           EpiMishBN{stem_.conv.b, stem_.sc, stem_.sh, x, (long)h * w * ldx, ldx}, st);
  for (int i = 0; i < last_stage; ++i) {
    const Res& r = res_[i];
    const int cin = kVaeChannels[i], cout = kVaeChannels[i + 1];
    const int mode = conv_mode(cin);
    const int ldo = vae_pix_channels(cout);
    const int oh = conv_out(h, 3, 2, 1), ow = conv_out(w, 3, 2, 1);
    ATDN_CHECK(r.a.conv.C == ldx && r.b.conv.C == ldx && r.skip.C == ldx, "channel layout mismatch between VAE layers");
    // every layer writes all ld channels of a pixel: the next one reads nothing that this call has not written
    ATDN_CHECK(r.a.conv.N == ldx && r.b.conv.N == ldo && r.skip.N == ldo, "channel layout mismatch between VAE layers");
    ATDN_CHECK(oh == plan_.h[i + 1] && ow == plan_.w[i + 1] && ldo == plan_.ld[i + 1] && conv_out(h, 1, 2, 0) == oh &&
               conv_out(w, 1, 2, 0) == ow, "layer plan and convolution geometry disagree");
    ATDN_CHECK(fits(bufB_, h, w, ldx), "MappingVAE scratch buffer too small for conv.0 of a residual block");
    run_conv(mode, shape(r.a.conv, x, h, w, 1, 1), EpiMishBN{r.a.conv.b, r.a.sc, r.a.sh, t, (long)h * w * ldx, ldx}, st);
    ATDN_CHECK(fits(bufS_, oh, ow, ldo), "MappingVAE scratch buffer too small for the skip convolution of a residual block");
    run_conv(mode, shape(r.skip, x, h, w, 2, 0), EpiBias<ACT_NONE>{r.skip.b, bufS_.p, (long)oh * ow * ldo, ldo, 1.f}, st);
    // x is dead after the skip conv: the block output overwrites it
    ATDN_CHECK(fits(bufA_, oh, ow, ldo), "MappingVAE scratch buffer too small for the output of a residual block");
    run_conv(mode, shape(r.b.conv, t, h, w, 2, 1),
             EpiMishBNSkipMishBN{r.b.conv.b, r.b.sc, r.b.sh, bufS_.p, (long)oh * ow * ldo, ldo, r.sc, r.sh, x,
                                 (long)oh * ow * ldo, ldo}, st);
    h = oh; w = ow; ldx = ldo;
  }
  if (!mu) return;
  ATDN_CHECK(last_stage == kVaeStages - 1 && h == oh_ && w == ow_ && ldx == 128, "unexpected encoder output geometry");
  conv_dispatch<MODE_TAP>(shape(mean_, x, h, w, 1, 0), EpiBias<ACT_NONE>{mean_.b, mu, (long)h * w * 128, 128, 1.f}, st);
}

}  // namespace atdn
