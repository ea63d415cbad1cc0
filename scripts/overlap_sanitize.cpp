// overlap_sanitize.cpp — the volume queries' host side (csrc/rt_overlap.hpp: host_overlap, with rt_multihit.hpp's
// host_tree_ok; what rt_host_overlap_volumes calls once its arguments are checked) under ASan and UBSan, host only, no
// GPU: triangle counts 0 to 100,000 through both builders of csrc/rt_lbvh.hpp and the flat definition; random, degenerate
// (a point, b = a, c on ab), non-finite, 1e37-scaled and 1e-30-scaled triangles; boxes around the triangles, point boxes,
// inverted, NaN, infinite and huge ones; balls at and around the triangles with every class of cap, NaN, infinite and
// far-away centres; cursors (a record, a miss record, NaN); every k from 0 to 16 with and without counts; damaged trees,
// which must be refused. Checks what must hold for every input: the walk returns the flat definition's bytes and counts,
// the records are ascending in (d2, prim), below the cap and beyond the cursor, unused records are the miss record, a
// smaller k is a prefix, and a query without hits by definition has none. Exit status 0 and "clean".
//
// (clang++: the headers use _Float16, which g++ has from version 12 on)
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I hello-raytracing_amd/csrc scripts/overlap_sanitize.cpp -o /tmp/overlap_sanitize && /tmp/overlap_sanitize
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "rt_lbvh.hpp"
#include "rt_overlap.hpp"

namespace O = hrt_overlap;

static O::Tree tree_of(const hrt_lbvh::HostTree& T, const std::vector<float>& geo, uint32_t m, bool flat) {
    O::Tree t{};
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

static bool is_miss(const O::Hit& h) {
    const O::Hit miss{O::T_MISS, -1, 0.0f, 0.0f};
    return std::memcmp(&h, &miss, sizeof h) == 0;
}

int main() {
    std::mt19937 g(23);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float caps[] = {nan, 0.0f, -0.0f, -1.0f, inf, std::numeric_limits<float>::max(), 1e-5f, 0.5f, 3.0f, 1e30f};
    const uint32_t sizes[] = {0u, 1u, 2u, 3u, 4u, 5u, 64u, 65u, 1025u, 100000u};
    unsigned long long records = 0, hits = 0, by_walk = 0;
    for (uint32_t m : sizes) {
        for (int shape = 0; shape < 6; shape++) {
            if (m == 100000u && shape > 1) continue;
            const float scale = shape == 4 ? 1e37f : shape == 5 ? 1e-30f : 1.0f;
            std::vector<float> geo(9 * (size_t)m);
            for (uint32_t j = 0; j < m; j++) {
                float* t = &geo[9 * (size_t)j];
                for (int k = 0; k < 3; k++) {
                    t[k] = 4.0f * scale * U(g);
                    t[3 + k] = 0.6f * scale * U(g);
                    t[6 + k] = 0.6f * scale * U(g);
                }
                if (shape == 1 && j % 3 == 0)                         // collapsed to a point
                    for (int k = 3; k < 9; k++) t[k] = 0.0f;
                if (shape == 1 && j % 3 == 1)                         // b = a
                    for (int k = 3; k < 6; k++) t[k] = 0.0f;
                if (shape == 1 && j % 3 == 2)                         // c on the line ab
                    for (int k = 0; k < 3; k++) t[6 + k] = 0.5f * t[3 + k];
                if (shape == 2 && j % 4 == 0) t[g() % 9u] = (j % 8 == 0) ? nan : inf;
                if (shape == 3) t[g() % 9u] = 0.0f;
            }
            const uint32_t n = m == 100000u ? 24u : 80u;
            hrt_lbvh::HostTree trees[2] = {hrt_lbvh::host_build(geo.data(), m, 0u), hrt_lbvh::host_build(geo.data(), m, 1u)};
            for (uint32_t kind = O::KIND_BOX; kind <= O::KIND_BALL; kind++) {
                const uint32_t w = O::volume_floats(kind);
                std::vector<float> vol(w * (size_t)n);
                std::vector<uint8_t> none(n, 0);  // no hits by definition
                for (uint32_t i = 0; i < n; i++) {
                    float c[3] = {4.0f * scale * U(g), 4.0f * scale * U(g), 4.0f * scale * U(g)};
                    if (m && i % 3 != 0) {  // at a triangle: its centroid, or a vertex
                        const float* t = &geo[9 * (size_t)(g() % m)];
                        const float wt = i % 2 ? 1.0f / 3.0f : 0.0f;
                        for (int k = 0; k < 3; k++) c[k] = t[k] + wt * (t[3 + k] + t[6 + k]);
                    }
                    float* v = &vol[w * (size_t)i];
                    if (kind == O::KIND_BOX) {
                        for (int k = 0; k < 3; k++) {
                            const float h = i % 5 == 0 ? 0.0f : scale * std::exp(3.0f * U(g) - 2.0f);  // a point box, or 0.7 % to 2.7
                            v[k] = c[k] - h;
                            v[3 + k] = c[k] + h;
                        }
                        if (i % 17 == 2) for (int k = 0; k < 3; k++) { v[k] = -3e38f; v[3 + k] = 3e38f; }  // huge: everything
                        if (i % 11 == 3) { v[g() % 6u] = (i % 4 == 1) ? nan : ((i % 4 == 2) ? inf : -inf); none[i] = 1; }
                        if (i % 13 == 5) { const int k = g() % 3u; v[k] = 1.0f * scale; v[3 + k] = -1.0f * scale; none[i] = 1; }
                    } else {
                        for (int k = 0; k < 3; k++) v[k] = c[k];
                        v[3] = caps[g() % (sizeof caps / sizeof caps[0])];
                        if (i % 7 == 0) v[3] = scale * scale * std::exp(4.0f * U(g) - 3.0f);
                        if (i % 17 == 2) v[g() % 3u] = 3e38f;   // D overflows: the loop over all triangles
                        if (i % 19 == 4) for (int k = 0; k < 3; k++) v[k] = 1e-42f * U(g);
                        if (i % 11 == 3) { v[g() % 3u] = (i % 4 == 1) ? nan : -inf; none[i] = 1; }
                        if (!(hrt_closest::cap_of(v[3]) > 0.0f)) none[i] = 1;
                    }
                }
                for (uint32_t builder = 0; builder < 2u; builder++) {
                    const hrt_lbvh::HostTree& T = trees[builder];
                    const size_t slots = T.hnodes.size() / 2;
                    O::Tree walk = tree_of(T, geo, m, false), flat = tree_of(T, geo, m, true);
                    if (!hrt_multihit::host_tree_ok(walk, slots, T.order.size())) return std::printf("a built tree was refused\n"), 1;
                    for (int pass = 0; pass < 2; pass++) {  // free; cursors
                        std::vector<O::Hit> full((size_t)n * O::MAX_K), cursor;
                        std::vector<uint32_t> fc(n), wc(n);
                        O::host_overlap(flat, kind, vol.data(), nullptr, n, O::MAX_K, full.data(), fc.data());
                        if (pass == 1) {
                            cursor.resize(n);
                            for (uint32_t i = 0; i < n; i++) {
                                cursor[i] = full[(size_t)i * O::MAX_K + (i % 3)];  // a record of the query, or the miss record
                                if (i % 13 == 6) cursor[i].d2 = nan;
                            }
                            O::host_overlap(flat, kind, vol.data(), cursor.data(), n, O::MAX_K, full.data(), fc.data());
                        }
                        const O::Hit* cur = pass == 1 ? cursor.data() : nullptr;
                        for (uint32_t k = 0; k <= O::MAX_K; k++) {
                            for (int counted = 0; counted < 2; counted++) {
                                if (k == 0 && !counted) continue;
                                std::vector<O::Hit> got((size_t)n * k);
                                O::host_overlap(walk, kind, vol.data(), cur, n, k, got.data(), counted ? wc.data() : nullptr);
                                for (uint32_t i = 0; i < n; i++) {
                                    const O::Hit* want = &full[(size_t)i * O::MAX_K];  // (a smaller k is a prefix)
                                    const O::Hit* have = got.data() + (size_t)i * k;
                                    records += k;
                                    if (k && std::memcmp(have, want, k * sizeof(O::Hit)) != 0)
                                        return std::printf("walk != flat: m %u shape %d kind %u builder %u pass %d k %u query %u\n", m, shape, kind, builder, pass, k, i), 1;
                                    if (counted && wc[i] != fc[i])
                                        return std::printf("counts differ: m %u shape %d kind %u builder %u pass %d k %u query %u: %u != %u\n", m, shape, kind, builder, pass, k, i, wc[i], fc[i]), 1;
                                }
                            }
                        }
                        for (uint32_t i = 0; i < n; i++) {  // what must hold of the flat answer itself
                            const O::Hit* h = &full[(size_t)i * O::MAX_K];
                            const float cap = kind == O::KIND_BALL ? hrt_closest::cap_of(vol[w * (size_t)i + 3]) : 1.0f;
                            const uint32_t listed = fc[i] < O::MAX_K ? fc[i] : O::MAX_K;
                            if (none[i] && fc[i] != 0u) return std::printf("a query without hits by definition has some\n"), 1;
                            for (uint32_t s = 0; s < O::MAX_K; s++) {
                                if (s >= listed) {
                                    if (!is_miss(h[s])) return std::printf("an unused record is not the miss record\n"), 1;
                                    continue;
                                }
                                hits++;
                                bool good = h[s].prim >= 0 && (uint32_t)h[s].prim < m && h[s].d2 >= 0.0f && h[s].d2 < cap;
                                if (kind == O::KIND_BOX) good = good && h[s].d2 == 0.0f && h[s].v == 0.0f && h[s].w == 0.0f;
                                else good = good && h[s].v >= 0.0f && h[s].w >= 0.0f && h[s].v + h[s].w <= 1.0f;
                                if (s) good = good && hrt_multihit::hit_less(h[s - 1].d2, h[s - 1].prim, h[s].d2, h[s].prim);
                                if (cur) good = good && hrt_multihit::hit_less(cur[i].d2, cur[i].prim, h[s].d2, h[s].prim);
                                if (!good) return std::printf("bad record: m %u shape %d kind %u pass %d query %u rank %u\n", m, shape, kind, pass, i, s), 1;
                                if (slots) by_walk++;
                            }
                        }
                    }
                    if (slots >= 2 && kind == O::KIND_BOX) {  // damaged trees are refused, not read past their arrays
                        std::vector<hrt_lbvh::U4> nodes = T.hnodes;
                        walk.hnodes = nodes.data();
                        nodes[1].w = nodes[0].w;  // a child named twice (or the same leaf twice: still a tree)
                        const bool twice = (nodes[0].w & O::LEAF_BIT) == 0u;
                        if (hrt_multihit::host_tree_ok(walk, slots, T.order.size()) == twice) return std::printf("twice\n"), 1;
                        nodes = T.hnodes;
                        nodes[1].w = (uint32_t)slots;  // past the slots
                        if (hrt_multihit::host_tree_ok(walk, slots, T.order.size())) return std::printf("past the slots\n"), 1;
                        nodes[1].w = O::LEAF_BIT | (uint32_t)T.order.size() << 4 | 1u;  // a leaf past the order
                        if (hrt_multihit::host_tree_ok(walk, slots, T.order.size())) return std::printf("past the order\n"), 1;
                        walk.hnodes = T.hnodes.data();
                        walk.m = m ? m - 1u : 0u;  // an order entry past the triangles (some leaf names the last one)
                        if (hrt_multihit::host_tree_ok(walk, slots, T.order.size()) && shape != 2) return std::printf("past m\n"), 1;
                    }
                }
            }
        }
    }
    std::printf("clean: %llu records compared, %llu hits checked, %llu of them on a tree with nodes\n", records, hits, by_walk);
    return by_walk > 1000 ? 0 : 1;
}
