// Stand-alone check of the host form of forward interpolation (atdn_vslam_amd/csrc/warm_start_host.h) for sanitizer builds:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/diag/warm_start_host_check.cpp -o check
//   ./check CASES.bin
// CASES.bin (tools/diag/*.bin is not kept in git) holds, per case, int32 h, int32 w, then the input flow and the expected output,
// each 2*h*w float32 — written from tests/golden/warm_start.npz:
//   python -c "import numpy as np; g=np.load('tests/golden/warm_start.npz'); f=open('CASES.bin','wb');
//              [(np.array(g['in_'+n].shape[1:],'i4').tofile(f), g['in_'+n].tofile(f), g['out_'+n].tofile(f)) for n in g['names'][:2]]"
// Each case is run alone and as a batch of two copies, with input and output in exactly sized heap blocks, so that a read or
// write past either end is caught. Exit status 0 = every output bit equals the expected one and no sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../atdn_vslam_amd/csrc/warm_start_host.h"

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s CASES.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t hw[2];
  int ncase = 0;
  while (fread(hw, sizeof(int32_t), 2, f) == 2) {
    const int h = hw[0], w = hw[1];
    const size_t n = (size_t)2 * h * w;
    std::vector<float> in(n), want(n);
    if (fread(in.data(), sizeof(float), n, f) != n || fread(want.data(), sizeof(float), n, f) != n) { fprintf(stderr, "short file\n"); return 2; }
    for (int B = 1; B <= 2; ++B) {
      float* src = new float[n * B];
      float* dst = new float[n * B];
      for (int b = 0; b < B; ++b) memcpy(src + n * b, in.data(), n * sizeof(float));
      atdn::forward_interpolate_host(src, B, h, w, dst);
      for (int b = 0; b < B; ++b)
        if (memcmp(dst + n * b, want.data(), n * sizeof(float)) != 0) { fprintf(stderr, "case %d (%dx%d) B=%d: output differs\n", ncase, h, w, B); return 1; }
      delete[] src;
      delete[] dst;
    }
    printf("case %d: %d x %d ok (B = 1, 2)\n", ncase, h, w);
    ++ncase;
  }
  fclose(f);
  if (!ncase) { fprintf(stderr, "no cases\n"); return 2; }
  // no valid source at all: zeros
  std::vector<float> in(2 * 6 * 9, -1000.0f), out(2 * 6 * 9, 1.0f);
  atdn::forward_interpolate_host(in.data(), 1, 6, 9, out.data());
  for (float v : out) if (v != 0.0f) { fprintf(stderr, "all-invalid case: non-zero output\n"); return 1; }
  printf("%d cases and the all-invalid case ok\n", ncase);
  return 0;
}
