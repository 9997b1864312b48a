// Stand-alone check of the host form of the flow-track rule (atdn_vslam_amd/csrc/flow_track_host.h) for sanitizer builds; needs no
// input file:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/diag/flow_track_host_check.cpp -o check
//   ./check
// Inputs and outputs sit in exactly sized heap blocks, so a read or write past either end is caught. Closed forms (6 x 12):
//   zero flow: everything stays alive with acc = 0;   a constant flow of (0.75, -0.5): acc is the running sum, and a track is
//   alive exactly while every position it stood on was inside;   R = I, t = (0.25 k, 0, 0), fx = 64, flow (-2, 0) per step: the
//   plane at depth 8 at every step;   a dead pixel stays dead under a flow that would carry it back, its acc bits kept;
//   NaN and infinite flows: every track dies and keeps its acc.
// Pseudo-random sequences of 4 steps at 5 x 7 (B = 1) and 9 x 33 (B = 3: H * W = 297 is odd, so the planes of b = 1, 2 start at
// odd offsets), with a mask, out of place and in place (the same bits), full form and chain-only form (the same chain): the
// counts are ordered, alive never grows, alive_out is 0 or 1, and a dead pixel keeps its acc and its depth.
// Exit status 0 = every expectation met and no sanitizer report.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../atdn_vslam_amd/csrc/flow_track_host.h"

using atdn::TwoViewCamera;

static const TwoViewCamera kPlane{64.0, 64.0, 5.0, 2.0, 1.0, 7.6e-7, 80.0};

// `steps` steps of the constant flow (u, v) from a fresh track, pose t = (t0 * k, 0, 0) after step k (t0 = 0: chain only)
static int closed(const char* name, float u, float v, float t0, int steps) {
  const int B = 2, H = 6, W = 12;
  const size_t n = (size_t)H * W;
  float* flow = new float[B * 2 * n];
  float* acc = new float[B * 2 * n]();
  unsigned char* alive = new unsigned char[B * n];
  float* pose = new float[B * 12];
  float* depth = new float[B * n]();
  int* counts = new int[B * 4];
  bool* ok = new bool[n];
  for (int b = 0; b < B; ++b)
    for (size_t i = 0; i < n; ++i) { flow[(2 * b) * n + i] = u; flow[(2 * b + 1) * n + i] = v; }
  memset(alive, 1, B * n);
  for (size_t i = 0; i < n; ++i) ok[i] = true;
  int bad = 0;
  for (int k = 0; k < steps; ++k) {
    for (int b = 0; b < B; ++b) {
      const float P[12] = {1, 0, 0, t0 * (k + 1), 0, 1, 0, 0, 0, 0, 1, 0};
      memcpy(pose + 12 * b, P, sizeof P);
    }
    for (int i = 0; i < B * 4; ++i) counts[i] = -12345;
    atdn::flow_track_step_host(flow, nullptr, acc, alive, B, H, W, acc, alive, t0 != 0.0f ? pose : nullptr, kPlane,
                               t0 != 0.0f ? depth : nullptr, counts);
    int want_alive = 0, want_valid = 0;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const double px = x + (double)u * k, py = y + (double)v * k;          // where the track stood before this step
        const bool fin = std::isfinite(u) && std::isfinite(v);
        ok[y * W + x] = ok[y * W + x] && fin && px >= 0 && px <= W - 1 && py >= 0 && py <= H - 1;
        want_alive += ok[y * W + x];
        const double qx = x + (double)u * (k + 1), qy = y + (double)v * (k + 1);
        want_valid += ok[y * W + x] && qx >= 0 && qx <= W - 1 && qy >= 0 && qy <= H - 1;
      }
    for (int b = 0; b < B; ++b) {
      if (counts[4 * b] != want_alive) { fprintf(stderr, "%s step %d: %d alive, expected %d\n", name, k, counts[4 * b], want_alive); ++bad; }
      if (t0 != 0.0f && (counts[4 * b + 1] != want_valid || counts[4 * b + 3] != want_valid)) {
        fprintf(stderr, "%s step %d: counts (%d, %d, %d), expected %d\n", name, k, counts[4 * b + 1], counts[4 * b + 2], counts[4 * b + 3], want_valid);
        ++bad;
      }
      for (size_t i = 0; i < n; ++i) {
        if (alive[b * n + i] != (ok[i] ? 1 : 0)) ++bad;
        if (ok[i] && (acc[(2 * b) * n + i] != u * (k + 1) || acc[(2 * b + 1) * n + i] != v * (k + 1))) ++bad;
        const float d = depth[b * n + i];
        if (t0 != 0.0f && d != 0.0f && !(std::fabs(d - 8.0f) <= 8.0f * 1.2e-7f)) ++bad;
      }
    }
  }
  delete[] flow; delete[] acc; delete[] alive; delete[] pose; delete[] depth; delete[] counts; delete[] ok;
  if (bad) fprintf(stderr, "%s: %d mismatches\n", name, bad); else printf("%s: %d steps ok\n", name, steps);
  return bad;
}

static int dead_stays_dead() {
  const int H = 6, W = 12;
  const size_t n = (size_t)H * W;
  float* flow = new float[2 * n];
  float* acc = new float[2 * n]();
  unsigned char* alive = new unsigned char[n];
  int counts[4];
  for (size_t i = 0; i < n; ++i) { flow[i] = 4.0f; flow[n + i] = 0.0f; }
  memset(alive, 200, n);                                          // any non-zero byte is alive
  const unsigned payload = 0x7FC12345u;
  memcpy(&acc[1 * W + 1], &payload, 4);
  alive[1 * W + 1] = 0;
  acc[2 * W + 3] = -5.0f;                                          // outside; +4 would bring it back
  alive[2 * W + 3] = 0;
  acc[3 * W + 0] = -1.5f;                                          // alive on entry, outside: dies now
  int bad = 0;
  for (int k = 0; k < 2; ++k) {
    atdn::flow_track_step_host(flow, nullptr, acc, alive, 1, H, W, acc, alive, nullptr, kPlane, nullptr, counts);
    unsigned bits;
    memcpy(&bits, &acc[1 * W + 1], 4);
    bad += bits != payload || alive[1 * W + 1] != 0 || alive[2 * W + 3] != 0 || acc[2 * W + 3] != -5.0f;
    bad += alive[3 * W + 0] != 0 || acc[3 * W + 0] != -1.5f;
    for (size_t i = 0; i < n; ++i) bad += alive[i] > 1;
  }
  delete[] flow; delete[] acc; delete[] alive;
  if (bad) fprintf(stderr, "dead pixels: %d mismatches\n", bad); else printf("dead pixels stay dead, ok\n");
  return bad;
}

static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static int random_case(int B, int H, int W) {
  const size_t n = (size_t)H * W;
  const int steps = 4;
  float* flow = new float[B * 2 * n];
  unsigned char* mask = new unsigned char[B * n];
  float* pose = new float[B * 12];
  // out of place: ping-pong buffers; in place: one set; chain only: one set
  float* acc[2] = {new float[B * 2 * n](), new float[B * 2 * n]};
  unsigned char* alive[2] = {new unsigned char[B * n], new unsigned char[B * n]};
  float* acc_ip = new float[B * 2 * n]();
  unsigned char* alive_ip = new unsigned char[B * n];
  float* acc_ch = new float[B * 2 * n]();
  unsigned char* alive_ch = new unsigned char[B * n];
  float* depth = new float[B * n]();
  float* depth_ip = new float[B * n]();
  float* depth_before = new float[B * n];
  int* counts = new int[B * 4];
  int* counts_ip = new int[B * 4];
  int* counts_ch = new int[B * 4];
  memset(alive[0], 1, B * n);
  memset(alive_ip, 1, B * n);
  memset(alive_ch, 1, B * n);
  unsigned s = 4321u + (unsigned)(H * W);
  const TwoViewCamera cam{4.0 * W / 7.0, 4.0 * W / 7.0, (W - 1) / 2.0 + 0.3, (H - 1) / 2.0 - 0.2, 1.0, 7.6e-7, 80.0};
  int bad = 0;
  int prev_alive[16];
  for (int b = 0; b < B; ++b) prev_alive[b] = (int)n;
  for (int k = 0; k < steps; ++k) {
    const int in = k & 1, out = in ^ 1;
    for (int b = 0; b < B; ++b) {
      const float P[12] = {1, 0, 0.01f, 0.05f * (b + 1) * (k + 1), 0, 1, 0, -0.02f * (k + 1), -0.01f, 0, 1, 1.0f * (k + 1)};
      memcpy(pose + 12 * b, P, sizeof P);
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          const size_t i = (size_t)y * W + x;
          const double z = 3.0 + 27.0 * (lcg(s) % 1000) / 1000.0;
          flow[(2 * b) * n + i] = (float)((x - cam.cx) / (z - 1.0) + ((int)(lcg(s) % 1500) - 750) / 1000.0);
          flow[(2 * b + 1) * n + i] = (float)((y - cam.cy) / (z - 1.0) + ((int)(lcg(s) % 1500) - 750) / 1000.0);
          mask[b * n + i] = (lcg(s) % 10) < 8 ? (unsigned char)(1 + lcg(s) % 255) : 0;
        }
    }
    memcpy(depth_before, depth, B * n * 4);
    atdn::flow_track_step_host(flow, mask, acc[in], alive[in], B, H, W, acc[out], alive[out], pose, cam, depth, counts);
    atdn::flow_track_step_host(flow, mask, acc_ip, alive_ip, B, H, W, acc_ip, alive_ip, pose, cam, depth_ip, counts_ip);
    atdn::flow_track_step_host(flow, mask, acc_ch, alive_ch, B, H, W, acc_ch, alive_ch, nullptr, cam, nullptr, counts_ch);
    bad += memcmp(acc[out], acc_ip, B * 2 * n * 4) != 0 || memcmp(alive[out], alive_ip, B * n) != 0;
    bad += memcmp(depth, depth_ip, B * n * 4) != 0 || memcmp(counts, counts_ip, B * 16) != 0;
    bad += memcmp(acc[out], acc_ch, B * 2 * n * 4) != 0 || memcmp(alive[out], alive_ch, B * n) != 0;
    for (int b = 0; b < B; ++b) {
      const int* c = counts + 4 * b;
      int live = 0;
      for (size_t i = 0; i < n; ++i) {
        const unsigned char a = alive[out][b * n + i];
        live += a;
        bad += a > 1 || (a && !alive[in][b * n + i]);
        if (!a) {
          bad += memcmp(&acc[out][(2 * b) * n + i], &acc[in][(2 * b) * n + i], 4) != 0;
          bad += memcmp(&acc[out][(2 * b + 1) * n + i], &acc[in][(2 * b + 1) * n + i], 4) != 0;
          bad += memcmp(&depth[b * n + i], &depth_before[b * n + i], 4) != 0;
        }
      }
      if (!(0 <= c[3] && c[3] <= c[2] && c[2] <= c[1] && c[1] <= c[0] && c[0] <= prev_alive[b]) || live != c[0]) ++bad;
      if (counts_ch[4 * b] != c[0] || counts_ch[4 * b + 1] || counts_ch[4 * b + 2] || counts_ch[4 * b + 3]) ++bad;
      prev_alive[b] = c[0];
      printf("random %d x %d b=%d step %d: counts (%d, %d, %d, %d)\n", H, W, b, k, c[0], c[1], c[2], c[3]);
    }
  }
  delete[] flow; delete[] mask; delete[] pose; delete[] acc[0]; delete[] acc[1]; delete[] alive[0]; delete[] alive[1];
  delete[] acc_ip; delete[] alive_ip; delete[] acc_ch; delete[] alive_ch; delete[] depth; delete[] depth_ip; delete[] depth_before;
  delete[] counts; delete[] counts_ip; delete[] counts_ch;
  if (bad) fprintf(stderr, "random %d x %d B = %d: %d mismatches\n", H, W, B, bad);
  return bad;
}

int main() {
  int bad = 0;
  bad += closed("zero flow", 0.f, 0.f, 0.f, 3);
  bad += closed("constant flow", 0.75f, -0.5f, 0.f, 5);
  bad += closed("plane", -2.f, 0.f, 0.25f, 3);
  bad += closed("nan flow", NAN, 0.f, 0.f, 2);
  bad += closed("inf flow", 0.f, -INFINITY, 0.f, 2);
  bad += dead_stays_dead();
  bad += random_case(1, 5, 7);
  bad += random_case(3, 9, 33);
  if (bad) { fprintf(stderr, "%d mismatches\n", bad); return 1; }
  printf("all cases ok\n");
  return 0;
}
