// Stand-alone check of the host forms of the visibility votes and the removal (atdn_vslam_amd/csrc/carve_host.h) for sanitizer
// builds; needs no input file:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/diag/carve_host_check.cpp -o check
//   ./check
// Points, depth, poses, indices, votes, keys, flags and the table sit in exactly sized heap blocks, so a read or write past
// either end is caught. Closed forms (9 x 11, fx = fy = 4, principal point (0, 0), R = I: a point at (u / 4 z, v / 4 z, z) has
// a = u + 0.5, b = v + 0.5; z = 2, rel 0.25 and abs 0.5 give lo = 1 and hi = 3): the window touching each border of the image
// at radius 0, 1, 2 and 8 and one pixel too far, the band's ends, an unmeasured and an equal-to-hi pixel in the window's
// corners, near and far and the next doubles outside, a point behind the camera, NaN and infinities in a point, in every slot
// of a pose and in the depth, index lists with repeats and entries outside the bank, M = 0, accumulation; then pseudo-random
// clouds at 5 x 7, 9 x 33 and 47 x 154 voted in one call and in three accumulated calls, which must agree. Removal: a table
// whose probe chains wrap around its end, absent and repeated keys, flags, R = 0, extraction, rehash and refill afterwards.
// Exit status 0 = every expectation met and no sanitizer report.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../atdn_vslam_amd/csrc/carve_host.h"

using namespace atdn;

static const float EYE[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
static const int HH = 9, WW = 11;

static int fail(const char* what) { fprintf(stderr, "FAILED: %s\n", what); return 1; }

static CarveParams hand(int radius, double rel = 0.25, double abs_tol = 0.5) {
  return carve_params(4.0, 4.0, 0.0, 0.0, 0.5, 40.0, rel, abs_tol, radius, HH, WW);
}

// one point seen at (u, v, z) by the hand camera (or `pose`) over a depth plane filled with `fill` and one pixel set
static int one(double u, double v, double z, const CarveParams& c, float fill = 8.0f, int py = -1, int px = -1, float pv = 0.0f,
               const float* pose = EYE) {
  float* pts = new float[3]{(float)(u / 4.0 * z), (float)(v / 4.0 * z), (float)z};
  float* depth = new float[HH * WW];
  float* P = new float[12];
  int* votes = new int[3];
  for (int i = 0; i < HH * WW; ++i) depth[i] = fill;
  if (py >= 0) depth[py * WW + px] = pv;
  memcpy(P, pose, 48);
  carve_votes_host(pts, 1, depth, P, nullptr, 1, 1, c, 0, votes);
  const int r = votes[0] | (votes[1] << 1) | (votes[2] << 2);
  delete[] pts; delete[] depth; delete[] P; delete[] votes;
  return r;
}

static int closed_forms() {
  int bad = 0;
  const int V = CARVE_VIEW, S = CARVE_SUPPORT, F = CARVE_FREE;
  for (int r : {0, 1, 2}) {
    if (one(r - 0.5, 4.0, 2.0, hand(r)) != (V | F)) bad += fail("left border in");
    if (one(r - 1.5, 4.0, 2.0, hand(r)) != 0) bad += fail("left border out");
    if (one(10.5 - r, 4.0, 2.0, hand(r)) != 0) bad += fail("right border out");
    if (one(9.5 - r, 4.0, 2.0, hand(r)) != (V | F)) bad += fail("right border in");
    if (one(5.0, r - 0.5, 2.0, hand(r)) != (V | F)) bad += fail("top border in");
    if (one(5.0, 8.5 - r, 2.0, hand(r)) != 0) bad += fail("bottom border out");
    if (one(5.0, 7.5 - r, 2.0, hand(r)) != (V | F)) bad += fail("bottom border in");
  }
  if (one(5.0, 4.0, 2.0, hand(8)) != 0) bad += fail("radius 8 does not fit 9 x 11");
  {
    float P[12];
    memcpy(P, EYE, 48);
    P[3] = ldexpf(1.0f, -54);                                       // a = the next double below 1
    if (one(0.5, 4.0, 2.0, hand(1), 8.0f, -1, -1, 0.0f, P) != 0) bad += fail("next double below the left border");
    P[3] = ldexpf(1.0f, -50);                                       // a = the next double below 10
    if (one(9.5, 4.0, 2.0, hand(1), 8.0f, -1, -1, 0.0f, P) != (V | F)) bad += fail("next double below the right border");
  }
  if (one(5.0, 4.0, 2.0, hand(1), 3.0f) != (V | S)) bad += fail("m == hi");
  if (one(5.0, 4.0, 2.0, hand(1), nextafterf(3.0f, 4.0f)) != (V | F)) bad += fail("m above hi");
  if (one(5.0, 4.0, 2.0, hand(1), 1.0f) != (V | S)) bad += fail("m == lo");
  if (one(5.0, 4.0, 2.0, hand(1), nextafterf(1.0f, 0.0f)) != V) bad += fail("m below lo");
  for (float pv : {0.0f, NAN, INFINITY, -INFINITY, -8.0f, 3.0f}) {
    if (one(5.0, 4.0, 2.0, hand(1), 8.0f, 3, 4, pv) != V) bad += fail("a corner of the window");
    if (one(5.0, 4.0, 2.0, hand(1), 8.0f, 5, 6, pv) != V) bad += fail("the opposite corner");
    if (one(5.0, 4.0, 2.0, hand(0), 8.0f, 3, 4, pv) != (V | F)) bad += fail("outside a radius-0 window");
  }
  if (one(5.0, 4.0, 2.0, hand(1), 8.0f, 4, 5, 0.0f) != V) bad += fail("unmeasured centre");
  if (one(5.0, 4.0, 2.0, hand(1), 40.0f) != (V | F)) bad += fail("m == far");
  if (one(5.0, 4.0, 2.0, hand(1), nextafterf(40.0f, 50.0f)) != V) bad += fail("m above far");
  if (one(5.0, 4.0, 0.5, hand(1, 0.0, 0.0), 0.5f) != (V | S)) bad += fail("m == near");
  if (one(5.0, 4.0, 0.5, hand(1, 0.0, 0.0), nextafterf(0.5f, 0.0f)) != V) bad += fail("m below near");
  if (one(5.0, 4.0, 0.5, hand(1), 0.0f) != V || one(5.0, 4.0, 40.0, hand(1), 0.0f) != V) bad += fail("z == near, z == far");
  {
    float P[12];
    memcpy(P, EYE, 48);
    P[11] = ldexpf(1.0f, -54);
    if (one(5.0, 4.0, 0.5, hand(1), 0.0f, -1, -1, 0.0f, P) != 0) bad += fail("z below near");
    P[11] = -ldexpf(1.0f, -47);
    if (one(5.0, 4.0, 40.0, hand(1), 0.0f, -1, -1, 0.0f, P) != 0) bad += fail("z above far");
  }
  if (one(5.0, 4.0, -2.0, hand(1)) != 0) bad += fail("behind the camera");
  for (float s : {NAN, INFINITY, -INFINITY})
    for (int k = 0; k < 12; ++k) {
      float P[12];
      memcpy(P, EYE, 48);
      P[k] = s;
      // (no component of d is 0 here, so every slot reaches c_0, c_1 or z)
      if (one(5.0, 4.0, 2.0, hand(1), 8.0f, -1, -1, 0.0f, P) != 0) bad += fail("special value in a pose");
    }
  if (!bad) printf("closed forms ok\n");
  return bad;
}

static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static int random_case(int H, int W, int N) {
  const int M = 4 * H * W;
  float* pts = new float[3 * M];
  float* depth = new float[(size_t)N * H * W];
  float* poses = new float[12 * N];
  unsigned r = 4711u + (unsigned)(H * W);
  for (int i = 0; i < M; ++i) {
    pts[3 * i] = -6.0f + 0.001f * (float)(lcg(r) % 12000);
    pts[3 * i + 1] = -2.0f + 0.001f * (float)(lcg(r) % 4000);
    pts[3 * i + 2] = -1.0f + 0.01f * (float)(lcg(r) % 4500);
  }
  pts[1] = NAN;
  pts[5] = INFINITY;
  const float odd[5] = {0.0f, NAN, INFINITY, -INFINITY, -1.0f};
  for (long i = 0; i < (long)N * H * W; ++i) depth[i] = lcg(r) % 7 == 0 ? odd[lcg(r) % 5] : 0.4f + 0.01f * (float)(lcg(r) % 4200);
  for (int k = 0; k < N; ++k) {
    const float P[12] = {1, 0, 0.02f * k, 0.3f * k, 0, 1, 0, -0.1f, -0.02f * k, 0, 1, -2.0f + 0.7f * k};
    memcpy(poses + 12 * k, P, sizeof P);
  }
  int bad = 0;
  for (int radius : {0, 1, 2, 8}) {
    const CarveParams c = carve_params(4.0 * W / 7.0, 4.0 * W / 7.0, (W - 1) / 2.0 + 0.3, (H - 1) / 2.0 - 0.2, 0.5, 40.0, 0.05, 0.25,
                                       radius, H, W);
    const int K = 2 * N + 3;
    int* ix = new int[K];
    for (int j = 0; j < K; ++j) ix[j] = j < 2 * N ? j % N : (j % 2 ? -1 : N);      // every keyframe twice, then outside the bank
    int* a = new int[3 * M];
    int* b = new int[3 * M];
    int* d = new int[3 * M];
    carve_votes_host(pts, M, depth, poses, ix, N, K, c, 0, a);
    carve_votes_host(pts, M, depth, poses, nullptr, N, N, c, 0, b);
    bool twice = true;
    long sums[3] = {0, 0, 0};
    for (int i = 0; i < 3 * M; ++i) {
      twice = twice && a[i] == 2 * b[i];
      sums[i % 3] += b[i];
    }
    if (!twice) bad += fail("every keyframe twice and entries outside the bank");
    for (int i = 0; i < 3 * M; ++i) d[i] = 7;
    const int cut1 = N / 3, cut2 = (2 * N + 2) / 3;                                // three calls over the list 0 .. N-1 (a part may be empty)
    carve_votes_host(pts, M, depth, poses, ix + cut2, N, N - cut2, c, 0, d);
    carve_votes_host(pts, M, depth, poses, ix, N, cut1, c, 1, d);
    carve_votes_host(pts, M, depth, poses, ix + cut1, N, cut2 - cut1, c, 1, d);
    bool split = true;
    for (int i = 0; i < 3 * M; ++i) split = split && d[i] == b[i];
    if (!split) bad += fail("split invariance");
    if (a[0] || a[1] || a[2] || a[3] || a[4] || a[5]) bad += fail("NaN and infinity in a point");
    carve_votes_host(nullptr, 0, depth, poses, nullptr, N, N, c, 0, nullptr);
    if (radius == 1) printf("random %d x %d, N = %d: votes (%ld, %ld, %ld)\n", H, W, N, sums[0], sums[1], sums[2]);
    delete[] ix; delete[] a; delete[] b; delete[] d;
  }
  delete[] pts; delete[] depth; delete[] poses;
  return bad;
}

static uint64_t key_of(long gx) { return ((uint64_t)(gx + 1048576) << 42) | ((uint64_t)1048576 << 21) | 1048576u; }

static int removal() {
  int bad = 0;
  const long cap = 64;
  uint64_t* table = new uint64_t[voxel_table_words(cap)];
  voxel_clear_host(table, cap);
  // 30 keys whose home slots are the last 8: the chains wrap around the table's end
  int64_t* keys = new int64_t[30];
  int n = 0;
  for (long g = 0; n < 30; ++g)
    if (voxel_home(key_of(g), (uint32_t)(cap - 1)) >= 56) keys[n++] = (int64_t)key_of(g);
  uint64_t* slots = table + VOX_HEADER_WORDS;
  for (int i = 0; i < 30; ++i) {
    bool fresh;
    const long s = voxel_find_host(slots, cap, (uint64_t)keys[i], &fresh);
    if (s < 0 || !fresh) bad += fail("insertion");
    slots[8 * s + 1] = (uint64_t)(i + 1);
    for (int k = 2; k < 8; ++k) slots[8 * s + k] = (uint64_t)(100 * i + k);
  }
  table[VOX_VOXELS] = 30;
  table[VOX_INSERTED] = table[VOX_CANDIDATES] = 465;
  int64_t* ask = new int64_t[12];
  for (int i = 0; i < 10; ++i) ask[i] = keys[3 * i];
  ask[10] = keys[3];
  ask[11] = (int64_t)key_of(999999);
  int64_t* removed = new int64_t[3];
  voxel_remove_host(table, cap, ask, nullptr, 12, removed);
  long want_points = 0;
  for (int i = 0; i < 10; ++i) want_points += 3 * i + 1;
  if (removed[0] != 10 || removed[1] != want_points || removed[2] != 2) bad += fail("removed counts");
  if (table[VOX_VOXELS] != 30 || table[VOX_INSERTED] != 465) bad += fail("the counters are not touched");
  unsigned char* flags = new unsigned char[12];
  memset(flags, 0, 12);
  flags[11] = 1;
  voxel_remove_host(table, cap, ask, flags, 12, removed);
  if (removed[0] != 0 || removed[1] != 0 || removed[2] != 1) bad += fail("flags");
  voxel_remove_host(table, cap, nullptr, nullptr, 0, removed);
  if (removed[0] || removed[1] || removed[2]) bad += fail("R = 0");
  // extraction skips the emptied voxels; a rehash carries them along; a later insertion finds their slots
  const VoxelParams p = voxel_params(1.0, 1.0, 0.0, 0.0, 1, 0.25, 0.0, 0.0, 0.0, 0.0, 0.0);
  float* pts = new float[3 * 30];
  unsigned char* rgb = new unsigned char[3 * 30];
  int* cnt = new int[30];
  int64_t* out_keys = new int64_t[30];
  int64_t* found = new int64_t[1];
  voxel_extract_host(table, cap, 1, p, 30, pts, rgb, cnt, out_keys, found);
  if (*found != 20) bad += fail("extraction after removal");
  const long big = 256;
  uint64_t* grown = new uint64_t[voxel_table_words(big)];
  voxel_clear_host(grown, big);
  voxel_rehash_host(table, cap, grown, big);
  voxel_extract_host(grown, big, 1, p, 30, pts, rgb, cnt, out_keys, found);
  if (*found != 20 || grown[VOX_VOXELS] != 30) bad += fail("rehash of an emptied table");
  const long s = voxel_lookup_host(grown + VOX_HEADER_WORDS, big, (uint64_t)keys[0]);
  if (s < 0 || grown[VOX_HEADER_WORDS + 8 * s + 1] != 0 || grown[VOX_HEADER_WORDS + 8 * s + 2] != 0) bad += fail("the emptied slot");
  if (voxel_lookup_host(grown + VOX_HEADER_WORDS, big, key_of(999999)) != -1) bad += fail("an absent key");
  delete[] table; delete[] keys; delete[] ask; delete[] removed; delete[] flags; delete[] pts; delete[] rgb; delete[] cnt;
  delete[] out_keys; delete[] found; delete[] grown;
  if (!bad) printf("removal ok\n");
  return bad;
}

int main() {
  int bad = closed_forms();
  bad += random_case(5, 7, 1);
  bad += random_case(9, 33, 3);
  bad += random_case(47, 154, 4);
  bad += removal();
  if (bad) { fprintf(stderr, "%d mismatches\n", bad); return 1; }
  printf("all cases ok\n");
  return 0;
}
