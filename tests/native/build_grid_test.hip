// TEST INFRASTRUCTURE ONLY: the builders' grid sizing (nex_amd/csrc/build_core.hpp
// build_tile_count, build_grid) on the host, no GPU call: one workgroup per
// tile of `tile` frames, refused when the tiles do not fit one grid
// (2^32 - 1 workgroups). Counts that give 0, 1, 2^32 - 1 and 2^32 tiles, and
// the largest count, for the builders' tile sizes (64 and 256 frames).
// Prints one line per failure and "ok <checks>" at the end; exit status 1 on any failure.
#include <stdio.h>

#include "../../nex_amd/csrc/build_core.hpp"

namespace {

int failures = 0;
unsigned checks = 0;

void expect_grid(uint64_t count, uint32_t tile, uint64_t want_tiles) {
    const uint64_t tiles = nexg::build_tile_count(count, tile);
    dim3 grid(77u, 5u, 3u);  // a refused count leaves it alone
    const hipError_t e = nexg::build_grid(count, tile, grid);
    const bool fits = want_tiles <= 0xFFFFFFFFull;
    const bool ok = tiles == want_tiles &&
                    (fits ? e == hipSuccess && grid.x == (uint32_t)want_tiles && grid.y == 1u && grid.z == 1u
                          : e == hipErrorInvalidValue && grid.x == 77u && grid.y == 5u && grid.z == 3u);
    checks++;
    if (ok) return;
    failures++;
    printf("FAIL count %llu tile %u: %llu tiles (want %llu), status %d, grid %u x %u x %u\n", (unsigned long long)count,
           tile, (unsigned long long)tiles, (unsigned long long)want_tiles, (int)e, grid.x, grid.y, grid.z);
}

}  // namespace

int main() {
    for (uint32_t tile : {64u, 256u}) {
        const uint64_t t = tile, most = 0xFFFFFFFFull;
        expect_grid(0, tile, 0);
        expect_grid(1, tile, 1);
        expect_grid(t, tile, 1);
        expect_grid(t + 1, tile, 2);
        expect_grid((most - 1) * t + 1, tile, most);  // the first and last counts of 2^32 - 1 tiles
        expect_grid(most * t, tile, most);
        expect_grid(most * t + 1, tile, most + 1);  // 2^32 tiles: refused
        expect_grid((most + 1) * t, tile, most + 1);
        expect_grid((1ull << 40) + 1, tile, ((1ull << 40) + 1 + t - 1) / t);
        expect_grid(~0ull, tile, ~0ull / t + 1);  // no overflow in the rounding
    }
    printf("ok %u\n", checks);
    return failures ? 1 : 0;
}
