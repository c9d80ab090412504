// Host-only check of the launch plan in gbrl_amd/csrc/leaf_accum.h (compiled with the address and undefined-behaviour sanitizers and run by
// tests/test_host.py): leaf_acc_plan at the edge of kStreamLdsBudget, its bounds on a sweep, and the numbers the launchers of refit.hip,
// newton.hip and predict_leaves.hip (k_leaf_counts) computed before they shared it, written down as literals.
#include "leaf_accum.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace gbrl::kern;

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("MISMATCH " __VA_ARGS__); std::printf("  (%s)\n", #cond); std::exit(1); } } while (0)

// the accumulators stop fitting behind the tile at one byte over the budget, wherever the bytes come from
static void check_budget_edge() {
    static_assert(kStreamLdsBudget == 159744, "156 KiB");
    const size_t tiles[] = {0, 256, 3328, 82176, kStreamLdsBudget - 8, kStreamLdsBudget - 1};
    for (size_t tile : tiles) {
        const size_t room = kStreamLdsBudget - tile;
        for (int over = -1; over <= 1; ++over) {
            if (over < 0 && room == 0) continue;
            const LeafAccPlan p = leaf_acc_plan(tile, room + over, 1000, 4, 256);
            CHECK(p.lds == kStreamLdsBudget + over, "tile %zu: lds %zu\n", tile, p.lds);
            CHECK(p.fits == (over <= 0), "tile %zu, %d bytes over: fits %d\n", tile, over, p.fits);
            CHECK(p.blocks == 256, "tile %zu: one block per CU at the budget, got %d\n", tile, p.blocks);   // 160 KiB / lds == 1, or 0 raised to 1
        }
    }
    const LeafAccPlan wide = leaf_acc_plan(kStreamLdsBudget + 1, 0, 10, 8, 256);   // the tile alone is too wide
    CHECK(!wide.fits && wide.blocks == 10, "tile over the budget: fits %d, blocks %d\n", wide.fits, wide.blocks);
    std::printf("budget edge: 6 tiles x one byte under, exact, one byte over\n");
}

// per_cu is never 0 (blocks >= 1 whenever there is a tile, also for lds == 0 and for lds far above a CU's LDS), blocks <= n_tiles, and
// blocks is n_tiles or a whole number of blocks per CU between 1 and the cap
static void check_bounds() {
    std::mt19937_64 rng(20240611);
    const size_t sizes[] = {0, 1, 64, 4096, 40959, 40960, 40961, 81920, 81921, 163839, 163840, 163841, 1u << 20, size_t(1) << 40};
    long plans = 0;
    for (size_t tile : sizes)
        for (size_t acc : sizes)
            for (int cap : {1, 4, 8})
                for (int cus : {1, 64, 256, 304})
                    for (int rep = 0; rep < 8; ++rep, ++plans) {
                        const int n_tiles = rep < 3 ? rep : 1 + static_cast<int>(rng() % (rep < 6 ? 3000 : 40000000));
                        const LeafAccPlan p = leaf_acc_plan(tile, acc, n_tiles, cap, cus);
                        CHECK(p.lds == tile + acc && p.fits == (tile + acc <= kStreamLdsBudget), "lds %zu + %zu\n", tile, acc);
                        CHECK(p.blocks <= n_tiles, "blocks %d > n_tiles %d\n", p.blocks, n_tiles);
                        CHECK(n_tiles < 1 || p.blocks >= 1, "blocks %d for n_tiles %d\n", p.blocks, n_tiles);
                        const int per_cu = p.blocks / cus;
                        CHECK(p.blocks == n_tiles || (p.blocks % cus == 0 && per_cu >= 1 && per_cu <= cap), "blocks %d, cus %d, cap %d\n", p.blocks, cus, cap);
                        const size_t lds = tile + acc;   // the blocks counted per CU hold their LDS in 160 KiB, unless that is the one block
                        CHECK(p.blocks == n_tiles || per_cu == 1 || per_cu * lds <= 160 * 1024, "per_cu %d x lds %zu\n", per_cu, lds);
                    }
    std::printf("bounds: %ld plans, per_cu never 0, 1 <= blocks <= n_tiles\n", plans);
}

// What the three launchers computed, each by its own copy of the expressions, on a 256-CU device -- evaluated by hand:
//   tile   refit, counts: 64 * (F | 1) * 4          newton: 64 * ((G * 8) | 1) * 4
//   acc    refit: leaves * (D + 1) * 8              newton: leaves * (2 D + 1) * 8          counts: counters * 4
//   per_cu = min(cap, max(1, 163840 / lds)), cap 4, 4, 8;  blocks = min(ceil(n / 64), 256 * per_cu);  fits = lds <= 159744
struct Row { char kind; int width, leaves, D, n; bool fits; size_t lds; int blocks; };
static const Row kRows[] = {
    {'r', 12, 16, 4, 3000, true, 3968, 47},            // 3328 + 640; per_cu 4; 47 tiles
    {'r', 100, 64, 64, 1000000, true, 59136, 512},     // 25856 + 33280; per_cu 2; 15625 tiles
    {'r', 300, 256, 32, 200000, true, 144640, 256},    // 77056 + 67584; per_cu 1; 3125 tiles
    {'r', 300, 512, 32, 200000, false, 212224, 256},   // 77056 + 135168: the general kernel
    {'r', 1, 2, 1, 1, true, 288, 1},                   // 256 + 32; one tile
    {'n', 1, 4, 1, 4097, true, 2400, 65},              // 2304 + 96; per_cu 4; 65 tiles
    {'n', 8, 64, 8, 1 << 20, true, 25344, 1024},       // 16640 + 8704; 163840 / 25344 = 6, capped at 4
    {'n', 32, 64, 64, 500000, true, 131840, 256},      // 65792 + 66048; per_cu 1; 7813 tiles
    {'n', 40, 128, 64, 500000, false, 214272, 256},    // 82176 + 132096: the general kernel
    {'c', 12, 4096, 0, 3000, true, 19712, 47},         // 3328 + 16384; per_cu 8; 47 tiles
    {'c', 64, 4096, 0, 1000000, true, 33024, 1024},    // 16640 + 16384; 163840 / 33024 = 4
    {'c', 500, 4096, 0, 100000, true, 144640, 256},    // 128256 + 16384; per_cu 1; 1563 tiles
    {'c', 620, 16, 0, 100, true, 159040, 2},           // 158976 + 64: the widest rows that fit; 2 tiles
    {'c', 624, 16, 0, 100, false, 160064, 2},          // 160000 + 64: the tile alone is over the budget
};
static void check_launchers() {
    for (const Row &r : kRows) {
        const size_t tile = static_cast<size_t>(64) * ((r.kind == 'n' ? r.width * 8 : r.width) | 1) * 4;
        const size_t acc = r.kind == 'c' ? static_cast<size_t>(r.leaves) * 4 : static_cast<size_t>(r.leaves) * ((r.kind == 'n' ? 2 : 1) * r.D + 1) * 8;
        const LeafAccPlan p = leaf_acc_plan(tile, acc, (r.n + 63) / 64, r.kind == 'c' ? 8 : 4, 256);
        CHECK(p.fits == r.fits && p.lds == r.lds && p.blocks == r.blocks, "%c width %d, leaves %d, D %d, n %d: fits %d, lds %zu, blocks %d\n", r.kind,
              r.width, r.leaves, r.D, r.n, p.fits, p.lds, p.blocks);
    }
    std::printf("launchers: %zu shapes of refit, newton and leaf counts reproduce their former numbers\n", sizeof(kRows) / sizeof(kRows[0]));
}

int main() {
    check_budget_edge();
    check_bounds();
    check_launchers();
    std::printf("leaf accumulators: all sections passed\n");
    return 0;
}
