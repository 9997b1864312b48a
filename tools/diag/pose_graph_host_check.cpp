// Stand-alone check of the host form of the pose-graph rule (atdn_vslam_amd/csrc/pose_graph_host.h) for sanitizer builds; needs no
// input file:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/diag/pose_graph_host_check.cpp -o check
//   ./check
// Inputs and outputs sit in exactly sized heap blocks, so a read or write past either end is caught. A ring of N poses about 1 m
// apart with exact measurements (the chain and two loops), a duplicate edge, a backward edge, a zero-weight edge and the three kinds
// of absent edge (an index -1, an index N, i == j); the start is pushed up to 0.3 m along x (0.05 m times k mod 7). With node 0 held, 8 steps must
// return within 1e-4 m of the truth; the held node must come back with its input bits; iters = 0 must return every input bit;
// the evaluation alone must give the solve's first cost. N = 7 and N = 300 (two chunks of the sum over nodes).
// Exit status 0 = every expectation met and no sanitizer report.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../atdn_vslam_amd/csrc/pose_graph_host.h"

static void truth_pose(int k, int N, double* T) {                 // rows of [R|t]: a turn about y, on a circle
  const double a = 2.0 * M_PI * k / N, r = N / (2.0 * M_PI);
  const double R[9] = {cos(a), 0, sin(a), 0, 1, 0, -sin(a), 0, cos(a)};
  const double t[3] = {r * sin(a), 0.1 * sin(3 * a), r * cos(a)};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[4 * i + j] = R[3 * i + j];
    T[4 * i + 3] = t[i];
  }
}

static void relative(const double* A, const double* B, float* Z) {   // A^-1 B
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Z[4 * i + j] = (float)(A[i] * B[j] + A[4 + i] * B[4 + j] + A[8 + i] * B[8 + j]);
    Z[4 * i + 3] = (float)(A[i] * (B[3] - A[3]) + A[4 + i] * (B[7] - A[7]) + A[8 + i] * (B[11] - A[11]));
  }
}

static int run(int N) {
  const int chain = N - 1, E = chain + 8;
  float* poses = new float[12 * N];
  int* index = new int[2 * E];
  float* meas = new float[12 * E];
  double* weight = new double[2 * E];
  unsigned char* robust = new unsigned char[E];
  unsigned char* fixed = new unsigned char[N];
  float* out = new float[12 * N];
  double* chi2 = new double[E];
  double cost[2], cost1[1];
  int counts[4], counts2[2];
  double* T = new double[12 * N];
  for (int k = 0; k < N; ++k) {
    truth_pose(k, N, T + 12 * k);
    for (int i = 0; i < 12; ++i) poses[12 * k + i] = (float)T[12 * k + i];
    poses[12 * k + 3] += 0.05f * (k % 7);
    fixed[k] = k == 0;
  }
  const int extra[8][2] = {{N - 1, 0}, {N / 2, 1}, {2, 3}, {5, 2}, {3, 6}, {-1, 2}, {1, N}, {4, 4}};
  for (int e = 0; e < E; ++e) {
    const int i = e < chain ? e : extra[e - chain][0], j = e < chain ? e + 1 : extra[e - chain][1];
    index[e] = i;
    index[E + e] = j;
    const bool ok = i >= 0 && i < N && j >= 0 && j < N;
    if (ok) relative(T + 12 * i, T + 12 * j, meas + 12 * e); else memset(meas + 12 * e, 0, 48);
    weight[2 * e] = e == chain + 4 ? 0.0 : 1e4;
    weight[2 * e + 1] = e == chain + 4 ? 0.0 : 1e2;
    robust[e] = e >= chain;
  }
  atdn::PgProblem P{poses, index, meas, weight, robust, fixed, N, E, 25.0};
  int bad = 0;
  atdn::pose_graph_run_host(P, 8, 64, 1e-8, out, cost, chi2, counts);
  double worst = 0.0;
  for (int k = 0; k < N; ++k)
    for (int i = 0; i < 3; ++i) worst = fmax(worst, fabs((double)out[12 * k + 4 * i + 3] - T[12 * k + 4 * i + 3]));
  printf("N %d: cost %.3g -> %.3g, %d accepted, %d CG iterations, worst |t - truth| %.2e m, edges %d valid %d absent\n", N, cost[0],
         cost[1], counts[2], counts[3], worst, counts[0], counts[1]);
  bad += !(worst < 1e-4) || counts[0] != E - 3 || counts[1] != 3 || counts[2] < 1 || memcmp(out, poses, 48) != 0;
  atdn::pose_graph_run_host(P, -1, 1, 1.0, nullptr, cost1, chi2, counts2);
  bad += cost1[0] != cost[0] || counts2[0] != E - 3 || chi2[chain + 5] != 0.0;
  atdn::pose_graph_run_host(P, 0, 64, 1e-8, out, cost, chi2, counts);
  bad += memcmp(out, poses, 48 * (size_t)N) != 0 || cost[0] != cost[1] || counts[2] != 0;
  delete[] poses; delete[] index; delete[] meas; delete[] weight; delete[] robust; delete[] fixed; delete[] out; delete[] chi2;
  delete[] T;
  return bad;
}

int main() {
  const int bad = run(7) + run(300);
  printf(bad ? "FAILED\n" : "ok\n");
  return bad != 0;
}
