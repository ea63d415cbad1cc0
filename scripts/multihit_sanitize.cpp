// multihit_sanitize.cpp — the multi-hit ray query's host side (csrc/rt_multihit.hpp: host_tree_ok and host_multi, what
// rt_host_cast_rays_multi calls once its arguments are checked) under ASan and UBSan, host only, no GPU: triangle counts 0
// to 100,000 through both builders of csrc/rt_lbvh.hpp and the flat definition; random, degenerate (a point, b = a, c on
// ab), non-finite, 1e37-scaled and 1e-30-scaled triangles; rays at the triangles, axis-parallel, zero, NaN, infinite, tiny
// and huge ones; every class of cap; cursors (a hit, a miss record, NaN); every k from 0 to 16 with and without counts;
// damaged trees, which must be refused. Checks what must hold for every input: the walk returns the flat definition's
// bytes and counts, the records are ascending in (t, prim) with 1e-4 <= t < cap and beyond the cursor, unused records are
// the miss record, a smaller k is a prefix, and a non-finite ray has no hits. Exit status 0 and "clean".
//
// (clang++: the headers use _Float16, which g++ has from version 12 on)
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I hello-raytracing_amd/csrc scripts/multihit_sanitize.cpp -o /tmp/multihit_sanitize && /tmp/multihit_sanitize
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "rt_lbvh.hpp"
#include "rt_multihit.hpp"

namespace M = hrt_multihit;

static M::Tree tree_of(const hrt_lbvh::HostTree& T, const std::vector<float>& geo, uint32_t m, bool flat) {
    M::Tree t{};
    t.hnodes = T.hnodes.data();
    t.order = T.order.data();
    t.geo = geo.data();
    t.m = m;
    t.root = T.root;
    t.flat = flat ? 1u : 0u;
    for (int k = 0; k < 3; k++) t.rc[k] = T.rc[k];
    t.rr_h = std::nextafter(T.radius * (1.0f + 0x1p-9f), INFINITY);
    return t;
}

static bool is_miss(const M::Hit& h) {
    const M::Hit miss{M::T_MISS, -1, 0.0f, 0.0f};
    return std::memcmp(&h, &miss, sizeof h) == 0;
}

int main() {
    std::mt19937 g(19);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float caps[] = {nan, 0.0f, -0.0f, -1.0f, inf, std::numeric_limits<float>::max(), 1e-5f, 0.5f, 3.0f, 1e30f};
    const uint32_t sizes[] = {0u, 1u, 2u, 3u, 4u, 5u, 64u, 65u, 1025u, 100000u};
    unsigned long long records = 0, hits = 0, by_walk = 0;
    for (uint32_t m : sizes) {
        for (int kind = 0; kind < 6; kind++) {
            if (m == 100000u && kind > 1) continue;
            const float scale = kind == 4 ? 1e37f : kind == 5 ? 1e-30f : 1.0f;
            std::vector<float> geo(9 * (size_t)m);
            for (uint32_t j = 0; j < m; j++) {
                float* t = &geo[9 * (size_t)j];
                for (int k = 0; k < 3; k++) {
                    t[k] = 4.0f * scale * U(g);
                    t[3 + k] = 0.6f * scale * U(g);
                    t[6 + k] = 0.6f * scale * U(g);
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
            const uint32_t n = m == 100000u ? 24u : 80u;
            std::vector<float> o(3 * (size_t)n), d(3 * (size_t)n), tmax(n);
            std::vector<uint8_t> finite(n, 1);
            for (uint32_t i = 0; i < n; i++) {
                for (int k = 0; k < 3; k++) o[3 * i + k] = 6.0f * scale * U(g);
                float target[3] = {4.0f * scale * U(g), 4.0f * scale * U(g), 4.0f * scale * U(g)};
                if (m && i % 3 != 0) {  // at a triangle: its centroid, or a vertex
                    const float* t = &geo[9 * (size_t)(g() % m)];
                    const float w = i % 2 ? 1.0f / 3.0f : 0.0f;
                    for (int k = 0; k < 3; k++) target[k] = t[k] + w * (t[3 + k] + t[6 + k]);
                }
                const float len = i % 7 == 0 ? 1e-3f : (i % 9 == 0 ? 1e4f : 1.0f);
                for (int k = 0; k < 3; k++) d[3 * i + k] = (target[k] - o[3 * i + k]) * len;
                if (i % 10 == 4) d[3 * i + g() % 3u] = 0.0f;                                   // axis-parallel
                if (i % 20 == 7) d[3 * i] = d[3 * i + 1] = d[3 * i + 2] = 0.0f;                // no direction
                if (i % 20 == 9) d[3 * i + g() % 3u] = 1e-35f;                                 // below the 1e-30 of inv
                if (i % 11 == 3) {
                    (i % 2 ? o : d)[3 * i + g() % 3u] = (i % 4 == 1) ? nan : -inf;
                    finite[i] = 0;
                }
                if (i % 17 == 2) o[3 * i + g() % 3u] = 3e38f;  // D overflows: no hits either
                tmax[i] = caps[g() % (sizeof caps / sizeof caps[0])];
            }
            hrt_lbvh::HostTree trees[2] = {hrt_lbvh::host_build(geo.data(), m, 0u), hrt_lbvh::host_build(geo.data(), m, 1u)};
            for (uint32_t builder = 0; builder < 2u; builder++) {
                const hrt_lbvh::HostTree& T = trees[builder];
                const size_t slots = T.hnodes.size() / 2;
                M::Tree walk = tree_of(T, geo, m, false), flat = tree_of(T, geo, m, true);
                if (!M::host_tree_ok(walk, slots, T.order.size())) return std::printf("a built tree was refused\n"), 1;
                for (int pass = 0; pass < 3; pass++) {  // no cap; caps; caps and cursors
                    const float* cap = pass ? tmax.data() : nullptr;
                    std::vector<M::Hit> full((size_t)n * M::MAX_K), cursor;
                    std::vector<uint32_t> fc(n), wc(n);
                    M::host_multi(flat, o.data(), d.data(), cap, nullptr, n, M::MAX_K, full.data(), fc.data());
                    if (pass == 2) {
                        cursor.resize(n);
                        for (uint32_t i = 0; i < n; i++) {
                            cursor[i] = full[(size_t)i * M::MAX_K + (i % 3)];  // a hit of the ray, or the miss record
                            if (i % 13 == 6) cursor[i].t = nan;
                        }
                        M::host_multi(flat, o.data(), d.data(), cap, cursor.data(), n, M::MAX_K, full.data(), fc.data());
                    }
                    const M::Hit* cur = pass == 2 ? cursor.data() : nullptr;
                    for (uint32_t k = 0; k <= M::MAX_K; k++) {
                        for (int counted = 0; counted < 2; counted++) {
                            if (k == 0 && !counted) continue;
                            std::vector<M::Hit> got((size_t)n * k);
                            M::host_multi(walk, o.data(), d.data(), cap, cur, n, k, got.data(), counted ? wc.data() : nullptr);
                            for (uint32_t i = 0; i < n; i++) {
                                const M::Hit* want = &full[(size_t)i * M::MAX_K];
                                const M::Hit* have = got.data() + (size_t)i * k;
                                records += k;
                                if (k && std::memcmp(have, want, k * sizeof(M::Hit)) != 0)
                                    return std::printf("walk != flat: m %u kind %d builder %u pass %d k %u ray %u\n", m, kind, builder, pass, k, i), 1;
                                if (counted && wc[i] != fc[i])
                                    return std::printf("counts differ: m %u kind %d builder %u pass %d k %u ray %u: %u != %u\n", m, kind, builder, pass, k, i, wc[i], fc[i]), 1;
                            }
                        }
                    }
                    for (uint32_t i = 0; i < n; i++) {  // what must hold of the flat answer itself
                        const M::Hit* h = &full[(size_t)i * M::MAX_K];
                        const float c = M::cap_of(cap ? cap[i] : M::T_MISS);
                        const uint32_t listed = fc[i] < M::MAX_K ? fc[i] : M::MAX_K;
                        if (!finite[i] && fc[i] != 0u) return std::printf("a non-finite ray has hits\n"), 1;
                        for (uint32_t s = 0; s < M::MAX_K; s++) {
                            if (s >= listed) {
                                if (!is_miss(h[s])) return std::printf("an unused record is not the miss record\n"), 1;
                                continue;
                            }
                            hits++;
                            bool good = h[s].prim >= 0 && (uint32_t)h[s].prim < m && h[s].t >= 1e-4f && h[s].t < c;
                            good = good && h[s].u >= 0.0f && h[s].v >= 0.0f && h[s].u + h[s].v <= 1.0f;
                            if (s) good = good && M::hit_less(h[s - 1].t, h[s - 1].prim, h[s].t, h[s].prim);
                            if (cur) good = good && M::hit_less(cur[i].t, cur[i].prim, h[s].t, h[s].prim);
                            if (!good) return std::printf("bad record: m %u kind %d pass %d ray %u rank %u\n", m, kind, pass, i, s), 1;
                            if (slots) by_walk++;
                        }
                    }
                }
                if (slots >= 2) {  // damaged trees are refused, not read past their arrays
                    std::vector<hrt_lbvh::U4> nodes = T.hnodes;
                    walk.hnodes = nodes.data();
                    nodes[1].w = nodes[0].w;  // a child named twice (or the same leaf twice: still a tree)
                    const bool twice = (nodes[0].w & M::LEAF_BIT) == 0u;
                    if (M::host_tree_ok(walk, slots, T.order.size()) == twice) return std::printf("twice\n"), 1;
                    nodes = T.hnodes;
                    nodes[1].w = (uint32_t)slots;  // past the slots
                    if (M::host_tree_ok(walk, slots, T.order.size())) return std::printf("past the slots\n"), 1;
                    nodes[1].w = M::LEAF_BIT | (uint32_t)T.order.size() << 4 | 1u;  // a leaf past the order
                    if (M::host_tree_ok(walk, slots, T.order.size())) return std::printf("past the order\n"), 1;
                    walk.hnodes = T.hnodes.data();
                    walk.m = m ? m - 1u : 0u;  // an order entry past the triangles (some leaf names the last one)
                    if (M::host_tree_ok(walk, slots, T.order.size()) && kind != 2) return std::printf("past m\n"), 1;
                }
            }
        }
    }
    std::printf("clean: %llu records compared, %llu hits checked, %llu of them on a tree with nodes\n", records, hits, by_walk);
    return by_walk > 1000 ? 0 : 1;
}
