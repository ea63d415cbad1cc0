// winding_sanitize.cpp — the winding-number query's host side (csrc/rt_winding.hpp: host_moments and host_winding, what
// rt_host_tree_moments and rt_host_winding_numbers call once their arguments are checked) under ASan and UBSan, host only,
// no GPU: triangle counts 0 to 100,000 through both builders of csrc/rt_lbvh.hpp and the flat definition; random,
// degenerate (a point, b = a, c on ab), non-finite, 1e37-scaled and 1e-30-scaled triangles; finite, NaN, infinite, far and
// on-vertex points; every class of beta; damaged trees, which must be refused. Checks what must hold for every input:
// finite input gives no NaN and no infinity, a non-finite point gives the quiet NaN, uncovered points and trees without
// nodes give the flat definition's bytes. Exit status 0 and "clean".
//
// (clang++: the headers use _Float16, which g++ has from version 12 on)
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I hello-raytracing_amd/csrc scripts/winding_sanitize.cpp -o /tmp/winding_sanitize && /tmp/winding_sanitize
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "rt_lbvh.hpp"
#include "rt_winding.hpp"

namespace W = hrt_winding;

static W::Tree tree_of(const hrt_lbvh::HostTree& T, const std::vector<float>& geo, uint32_t m, const std::vector<float>& mom) {
    W::Tree t{};
    t.hnodes = (const W::U4*)T.hnodes.data();
    t.moments = mom.data();
    t.order = T.order.data();
    t.geo = geo.data();
    t.m = m;
    t.root = T.root;
    for (int k = 0; k < 3; k++) t.rc[k] = T.rc[k];
    t.rr_h = std::nextafter(T.radius * (1.0f + 0x1p-9f), INFINITY);
    return t;
}

int main() {
    static_assert(sizeof(W::U4) == sizeof(hrt_lbvh::U4), "one node format");
    std::mt19937 g(18);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float betas[] = {0.0f, -0.0f, 1.0f, 2.0f, 3.0f, 1e30f, inf};
    const float bad_betas[] = {nan, -1.0f, -inf, 0.5f, 1e-40f};
    for (float b : betas)
        if (!W::beta_ok(b)) return std::printf("beta %g refused\n", (double)b), 1;
    for (float b : bad_betas)
        if (W::beta_ok(b)) return std::printf("beta %g taken\n", (double)b), 1;
    const uint32_t sizes[] = {0u, 1u, 2u, 3u, 4u, 5u, 64u, 65u, 1025u, 100000u};
    unsigned long long answers = 0, walked = 0;
    for (uint32_t m : sizes) {
        for (int kind = 0; kind < 6; kind++) {
            if (m == 100000u && kind > 1) continue;
            const float scale = kind == 4 ? 1e37f : kind == 5 ? 1e-30f : 1.0f;
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
            std::vector<float> pts(3 * (size_t)n);
            std::vector<uint8_t> finite(n, 1);
            for (uint32_t i = 0; i < n; i++) {
                const float reach = i % 5 == 0 ? 4000.0f : (i % 7 == 0 ? 1e25f : 4.0f);
                for (int k = 0; k < 3; k++) pts[3 * i + k] = reach * (kind == 4 ? 1e12f : scale) * U(g);
                if (kind == 4 && i % 5 != 0 && i % 7 != 0)
                    for (int k = 0; k < 3; k++) pts[3 * i + k] = 4.0f * scale * U(g);
                if (i % 11 == 3) {
                    pts[3 * i + g() % 3u] = (i % 2) ? nan : -inf;
                    finite[i] = 0;
                }
                if (i % 13 == 5 && m && finite[i]) {  // on a vertex
                    const float* t = &geo[9 * (size_t)(g() % m)];
                    bool ok = true;
                    for (int k = 0; k < 3; k++) ok = ok && std::isfinite(t[k]);
                    if (ok)
                        for (int k = 0; k < 3; k++) pts[3 * i + k] = t[k];
                }
            }
            W::Tree flat{};
            flat.geo = geo.data();
            flat.m = m;
            flat.root = W::LEAF_BIT;
            std::vector<float> wf(n), w(n);
            W::host_winding(flat, pts.data(), n, 0.0f, wf.data());
            for (uint32_t builder = 0; builder < 2u; builder++) {
                const hrt_lbvh::HostTree T = hrt_lbvh::host_build(geo.data(), m, builder);
                const size_t slots = T.hnodes.size() / 2;
                std::vector<float> mom(W::REC_FLOATS * (slots ? slots : 1));
                W::Tree t = tree_of(T, geo, m, mom);
                if (!W::host_moments(t, slots, T.order.size(), mom.data())) return std::printf("a built tree was refused\n"), 1;
                for (float mv : mom)
                    if (std::isinf(mv)) return std::printf("an infinite moment\n"), 1;
                for (float beta : betas) {
                    W::host_winding(t, pts.data(), n, beta, w.data());
                    for (uint32_t i = 0; i < n; i++) {
                        answers++;
                        uint32_t bits;
                        std::memcpy(&bits, &w[i], 4);
                        bool good = finite[i] ? std::isfinite(w[i]) : bits == 0x7FC00000u;
                        if (slots == 0 || kind >= 4) good = good && std::memcmp(&w[i], &wf[i], 4) == 0;
                        if (!good) {
                            std::printf("bad answer: m %u kind %d builder %u beta %g point %u: %g (flat %g)\n", m, kind, builder,
                                        (double)beta, i, (double)w[i], (double)wf[i]);
                            return 1;
                        }
                        if (slots && finite[i] && std::memcmp(&w[i], &wf[i], 4) != 0) walked++;
                    }
                }
                if (slots >= 2) {  // damaged trees are refused, not read past their arrays
                    std::vector<hrt_lbvh::U4> nodes = T.hnodes;
                    t.hnodes = (const W::U4*)nodes.data();
                    nodes[1].w = nodes[0].w;  // a child named twice (or the same leaf twice: still a tree)
                    const bool twice = (nodes[0].w & W::LEAF_BIT) == 0u;
                    if (W::host_moments(t, slots, T.order.size(), mom.data()) == twice) return std::printf("twice\n"), 1;
                    nodes = T.hnodes;
                    nodes[1].w = (uint32_t)slots;  // past the slots
                    if (W::host_moments(t, slots, T.order.size(), mom.data())) return std::printf("past the slots\n"), 1;
                    nodes[1].w = W::LEAF_BIT | (uint32_t)T.order.size() << 4 | 1u;  // a leaf past the order
                    if (W::host_moments(t, slots, T.order.size(), mom.data())) return std::printf("past the order\n"), 1;
                    t.hnodes = (const W::U4*)T.hnodes.data();
                    t.m = m ? m - 1u : 0u;  // an order entry past the triangles (some leaf names the last one)
                    if (W::host_moments(t, slots, T.order.size(), mom.data()) && kind != 2) return std::printf("past m\n"), 1;
                }
            }
        }
    }
    std::printf("clean: %llu answers, %llu of them by the walk\n", answers, walked);
    return walked > 1000 ? 0 : 1;
}
