// tile_lists_sanitize.cpp — the tile-list rule (csrc/rt_tile_lists.hpp) under ASan and UBSan, host only, no GPU:
// random views, row shares and sphere sets, with zero and negative focal lengths, NaN and infinite camera values, zero
// radii, one-pixel images and K = 0..8. Exit status 0 and "clean" when every list is well formed.
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I hello-raytracing_amd/csrc scripts/tile_lists_sanitize.cpp -o /tmp/tile_lists_sanitize && /tmp/tile_lists_sanitize
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "rt_tile_lists.hpp"

int main() {
    std::mt19937 g(13);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    const float odd[] = {0.0f, -1.0f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                         -std::numeric_limits<float>::infinity(), 1e-30f, 1e30f};
    unsigned long long tiles = 0, walk = 0, entries = 0;
    for (int view = 0; view < 400; view++) {
        hrt_tiles::View V{};
        const float far = (view % 7 == 0) ? 1e5f : 10.0f;
        for (int i = 0; i < 3; i++) {
            V.eye[i] = far * U(g);
            V.dir[i] = U(g);
            V.up[i] = U(g);
            V.right[i] = U(g);
        }
        V.dir[3] = (view % 3) ? 1.0f : 0.0f;
        V.focal = 1.0f + 9.0f * (0.5f + 0.5f * U(g));
        V.blur = (view % 4) ? 0.05f * U(g) : 0.0f;
        V.k = 0.05f + 0.3f * (0.5f + 0.5f * U(g));
        V.W = 1u + (uint32_t)(g() % 200u);
        V.H = 1u + (uint32_t)(g() % 120u);
        V.aspect = (float)V.W / (float)V.H;
        V.wm1 = (float)V.W - 1.0f;
        V.hm1 = (float)V.H - 1.0f;
        V.row_block = 1u + (uint32_t)(g() % 9u);
        const uint32_t ranks = 1u + (uint32_t)(g() % 8u);
        V.row_stride = V.row_block * ranks;
        V.row0 = V.row_block * (uint32_t)(g() % ranks);
        V.nrows = 0;
        for (uint32_t y = V.row0; y < V.H; y += V.row_stride)
            for (uint32_t k = 0; k < V.row_block && y + k < V.H; k++) V.nrows++;
        V.tiles_w = (V.W + 7u) / 8u;
        V.tiles_h = (V.nrows + 7u) / 8u;
        V.k_list = (uint32_t)(g() % (hrt_tiles::K_MAX + 1u));
        if (view % 5 == 0) {  // one odd value somewhere in the camera
            float* const slots[] = {&V.focal, &V.blur, &V.k, &V.eye[0], &V.dir[1], &V.up[2], &V.right[0], &V.wm1, &V.aspect};
            *slots[g() % 9u] = odd[g() % 7u];
        }
        const uint32_t nleaf = (uint32_t)(g() % 300u);
        std::vector<float> sph(4u * nleaf + 4u);
        for (uint32_t c = 0; c < nleaf; c++) {
            for (int i = 0; i < 3; i++) sph[4 * c + i] = V.eye[i] + 12.0f * U(g);
            const float r = (c % 17u == 0u) ? 0.0f : 0.02f + 0.5f * (0.5f + 0.5f * U(g));
            sph[4 * c + 3] = r * r;
        }
        for (uint32_t t = 0; t < V.tiles_w * V.tiles_h; t++) {
            uint32_t out[hrt_tiles::WORDS];
            hrt_tiles::tile_list(V, t, sph.data(), nleaf, out);
            tiles++;
            if (out[0] == hrt_tiles::WALK) {
                walk++;
                continue;
            }
            if (out[0] > V.k_list) return std::printf("view %d tile %u: %u entries, K %u\n", view, t, out[0], V.k_list), 1;
            for (uint32_t i = 0; i < out[0]; i++) {
                if (out[1 + i] >= nleaf || (i && out[1 + i] <= out[i]))
                    return std::printf("view %d tile %u: entry %u is %u\n", view, t, i, out[1 + i]), 1;
                entries++;
            }
        }
    }
    std::printf("clean: %llu tiles, %llu walk, %llu entries\n", tiles, walk, entries);
    return 0;
}
