// Microbenchmark: the sorted-run, register-accumulating histogram kernel (gbrl_amd/csrc/hist_sorted.h)
// against the production LDS-atomic kernel k_hist_build on the same inputs, partials compared bit for bit.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -I gbrl_amd/csrc scripts/hist_sorted_bench.hip gbrl_amd/csrc/step_hist_reduce.hip gbrl_amd/csrc/hooks.cpp -o scripts/bin/hist_sorted_bench
//   hist_sorted_bench [frac=1] [chunk_rows=32768] [skew=0]
//     frac > 1: a gathered subset of N / frac rows (levels >= 1); skew = 1: class sizes far from uniform (codes ~ u^3)
#include "../gbrl_amd/csrc/step_hist_build.hip"
#include "experiments/hist_sorted.h"
#include <cstdio>
#include <cstring>
#include <vector>
#include <random>
using namespace gbrl::kern;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)
int main(int argc, char **argv) {
    const int N = 1 << 20, F = 128, D = 8, NB = 257, FG = 16;
    const int frac = argc > 1 ? atoi(argv[1]) : 1;
    const int chunk_rows = argc > 2 ? atoi(argv[2]) : 32768;
    const int skew = argc > 3 ? atoi(argv[3]) : 0;
    const int n_groups = F / FG;
    std::mt19937 rng(1);
    std::vector<uint16_t> codes(size_t(N) * F);
    for (auto &c : codes) {
        if (!skew) c = rng() % NB;
        else { double u = (rng() % 100000) / 100000.0; c = uint16_t(u * u * u * NB); if (c >= NB) c = NB - 1; }
    }
    std::vector<int32_t> qg(size_t(N) * D);
    for (auto &q : qg) q = int(rng() % 60001) - 30000;
    const int M = N / frac;
    std::vector<int32_t> rows(M);
    for (int i = 0; i < M; ++i) rows[i] = frac == 1 ? i : (i * frac + int(rng() % frac));
    std::vector<Chunk> chunks;
    for (int off = 0; off < M; off += chunk_rows) chunks.push_back({0, off, std::min(chunk_rows, M - off), 0});
    uint16_t *dc; int32_t *dq, *dr, *dp, *dp2; Chunk *dk;
    const size_t n_acc = size_t(NB) * (D + 1) * FG;
    const size_t pbytes = chunks.size() * n_groups * n_acc * 4;
    CK(hipMalloc(&dc, codes.size() * 2)); CK(hipMalloc(&dq, qg.size() * 4)); CK(hipMalloc(&dr, rows.size() * 4));
    CK(hipMalloc(&dk, chunks.size() * sizeof(Chunk))); CK(hipMalloc(&dp, pbytes)); CK(hipMalloc(&dp2, pbytes));
    CK(hipMemcpy(dc, codes.data(), codes.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(dq, qg.data(), qg.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dr, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dk, chunks.data(), chunks.size() * sizeof(Chunk), hipMemcpyHostToDevice));
    CK(hipMemset(dp, 0, pbytes)); CK(hipMemset(dp2, 0xff, pbytes));
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    const double units = double(M) * F / 64.0;    // (row, feature) pairs in units of one wave-instruction
    for (int rep = 0; rep < 3; ++rep) {
        CK(hipEventRecord(a));
        hist_build(dc, N, dq, D, dr, dk, (int)chunks.size(), n_groups, FG, NB, dp, 0);
        CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
        float ms; CK(hipEventElapsedTime(&ms, a, b));
        printf("atomic  rows=%d chunks=%zu  %.1f us   (%.1f clk per 64 pairs per CU at 2.3 GHz)\n", M, chunks.size(), ms * 1e3,
               ms * 1e-3 * 2.3e9 * 256 / units);
    }
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_hist_sorted<8>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const int grid = 8 * n_groups * (((int)chunks.size() + 7) / 8);
    for (int rep = 0; rep < 3; ++rep) {
        CK(hipEventRecord(a));
        hipLaunchKernelGGL(k_hist_sorted<8>, dim3(grid), dim3(kSortThreads), hist_sorted_lds_bytes(NB, D), 0, dc, N, dq, dr, dk, (int)chunks.size(),
                           n_groups, NB, dp2);
        CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
        CK(hipGetLastError());
        float ms; CK(hipEventElapsedTime(&ms, a, b));
        printf("sorted  rows=%d chunks=%zu  %.1f us   (%.1f clk per 64 pairs per CU at 2.3 GHz)\n", M, chunks.size(), ms * 1e3,
               ms * 1e-3 * 2.3e9 * 256 / units);
    }
#ifdef HS_PROFILE
    { long long ph[8]; CK(hipMemcpyFromSymbol(ph, HIP_SYMBOL(hs_profile), sizeof(ph)));
      const double su = double(chunk_rows) * 16 / 64.0;
      printf("block 0 phases (clock64 ticks per 64 pairs; 100 MHz counter -> x23 for core clk): zero %.2f stage+rank %.2f scan %.2f scatter %.2f accumulate %.2f\n",
             ph[0] / su, ph[1] / su, ph[2] / su, ph[3] / su, ph[4] / su); }
#endif
    std::vector<int32_t> h1(pbytes / 4), h2(pbytes / 4);
    CK(hipMemcpy(h1.data(), dp, pbytes, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h2.data(), dp2, pbytes, hipMemcpyDeviceToHost));
    size_t bad = 0;
    for (size_t i = 0; i < h1.size(); ++i) bad += h1[i] != h2[i];
    printf("partials: %zu words, %zu differ -> %s\n", h1.size(), bad, bad ? "MISMATCH" : "bit-identical");
    return bad ? 2 : 0;
}
