// closest_sanitize.cpp — the point-query definition (csrc/rt_closest.hpp host_closest) under ASan and UBSan, host only, no
// GPU: triangle counts 0 to 100,000, random, degenerate (a point, b = a, c on ab), non-finite and 1e37-scaled triangles,
// finite, NaN and infinite points, every class of cap. Checks what must hold for every input: v >= 0, w >= 0, v + w <= 1,
// a d2 that is never NaN in a record, a miss record that is all zeros below prim. Exit status 0 and "clean".
//
// (clang++: rt_closest.hpp includes rt_lbvh.hpp, which uses _Float16; g++ has it from version 12 on)
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I hello-raytracing_amd/csrc scripts/closest_sanitize.cpp -o /tmp/closest_sanitize && /tmp/closest_sanitize
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "rt_closest.hpp"

int main() {
    std::mt19937 g(17);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float odd_caps[] = {nan, 0.0f, -0.0f, -1.0f, inf, std::numeric_limits<float>::max(), 1e-12f, 0.25f};
    const uint32_t sizes[] = {0u, 1u, 2u, 3u, 4u, 5u, 64u, 65u, 1025u, 100000u};
    unsigned long long records = 0, hits = 0;
    for (uint32_t m : sizes) {
        for (int kind = 0; kind < 5; kind++) {
            if (m == 100000u && kind > 1) continue;
            const float scale = kind == 4 ? 1e37f : 1.0f;
            std::vector<float> geo(9 * (size_t)m);
            for (uint32_t j = 0; j < m; j++) {
                float* t = &geo[9 * (size_t)j];
                for (int k = 0; k < 3; k++) {
                    t[k] = 4.0f * scale * U(g);
                    t[3 + k] = 0.3f * scale * U(g);
                    t[6 + k] = 0.3f * scale * U(g);
                }
                if (kind == 1 && j % 3 == 0)                         // collapsed to a point
                    for (int k = 3; k < 9; k++) t[k] = 0.0f;
                if (kind == 1 && j % 3 == 1)                         // b = a
                    for (int k = 3; k < 6; k++) t[k] = 0.0f;
                if (kind == 1 && j % 3 == 2)                         // c on the line ab
                    for (int k = 0; k < 3; k++) t[6 + k] = 0.5f * t[3 + k];
                if (kind == 2 && j % 4 == 0) t[g() % 9u] = (j % 8 == 0) ? nan : inf;
                if (kind == 3) t[g() % 9u] = 0.0f;
            }
            const uint32_t n = m == 100000u ? 16u : 96u;
            std::vector<float> pts(3 * (size_t)n), caps(n);
            for (uint32_t i = 0; i < n; i++) {
                for (int k = 0; k < 3; k++) pts[3 * i + k] = (i % 5 == 0 ? 4000.0f : 4.0f) * scale * U(g);
                if (i % 11 == 3) pts[3 * i + g() % 3u] = (i % 2) ? nan : -inf;
                if (i % 13 == 5 && m) {  // on a vertex
                    const float* t = &geo[9 * (size_t)(g() % m)];
                    for (int k = 0; k < 3; k++) pts[3 * i + k] = t[k];
                }
                caps[i] = (i % 3 == 0) ? odd_caps[(i / 3) % 8] : 16.0f * scale * scale * (0.5f + 0.5f * U(g));
            }
            for (int with_caps = 0; with_caps < 2; with_caps++) {
                std::vector<hrt_closest::Record> out(n);
                hrt_closest::host_closest(geo.data(), m, pts.data(), with_caps ? caps.data() : nullptr, n, out.data());
                for (uint32_t i = 0; i < n; i++) {
                    const hrt_closest::Record& r = out[i];
                    records++;
                    bool good = !std::isnan(r.d2) && r.reserved == 0u && r.v >= 0.0f && r.w >= 0.0f &&
                                (double)r.v + (double)r.w <= 1.0;
                    if (r.prim < 0) {
                        good = good && r.prim == -1 && r.d2 == hrt_closest::T_MISS && r.v == 0.0f && r.w == 0.0f &&
                               r.p[0] == 0.0f && r.p[1] == 0.0f && r.p[2] == 0.0f;
                    } else {
                        hits++;
                        const float cap = hrt_closest::cap_of(with_caps ? caps[i] : hrt_closest::T_MISS);
                        good = good && (uint32_t)r.prim < m && r.d2 >= 0.0f && r.d2 < cap && std::isfinite(r.p[0]) &&
                               std::isfinite(r.p[1]) && std::isfinite(r.p[2]);
                    }
                    if (!good) {
                        std::printf("bad record: m %u kind %d caps %d point %u: d2 %g prim %d v %g w %g\n", m, kind,
                                    with_caps, i, (double)r.d2, r.prim, (double)r.v, (double)r.w);
                        return 1;
                    }
                }
            }
        }
    }
    std::printf("clean: %llu records, %llu hits\n", records, hits);
    return hits > 1000 ? 0 : 1;
}
