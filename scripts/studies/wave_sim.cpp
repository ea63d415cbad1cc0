// wave_sim.cpp — STUDY (round 7), not product code. Wave-lockstep model of k_trace_split<LNODES> on a sphere scene
// (VERDICT r6 item 2): what the wave runs, not what its lanes take.
//
// One simulated wave of 64 lanes; each lane does what a real lane does in a round of the kernel:
//   refill  a lane without a sample takes the next entry of the wave's frame block, dealt by lane rank among the lanes
//           that need one; a used-up block is remade for the job's next frame by all 64 lanes (one wave event). A job is
//           a random 8x8 tile x `job_frames` consecutive frames (time 1000 + 10 f); entries outside the image are
//           consumed and give no sample.
//   begin   lanes that start a query (the large list, the slab constants).
//   walk    bvh_walk_noovf, step by step for the whole wave: outer iterations of descent -> leaf -> pop. The descent loop runs
//           while any lane wants another box step; `hold` > 0 is the descent hold (the wave leaves the loop after a step
//           that fewer than min(hold, lanes that entered the iteration) lanes would follow with another one; the
//           stragglers keep their node, skip the pop, and step in the next iteration). After the pop the walk is
//           suspended when fewer than `suspend_below` lanes still walk.
//           `chold` > 0 is the candidate hold priced in round 10 (never built): a lane whose leaf gave it a candidate keeps
//           its leaf word and its candidates and skips the pop; the wave runs the root pass only once at least `chold`
//           lanes of the call hold a candidate, or every lane of the call does, or a lane has waited `cwait` iterations.
//   shade   lanes whose walk has finished: the hit (the oracle's closest_sphere), then scatter or the sample's end.
//   `blocktime` 1 (round 13, BLOCKRES): a block made for a tile with a primary candidate list is answered and shaded by all
//           64 lanes when it is made: a miss ends its sample, a hit scatters, and the block's entries are the survivors,
//           compacted, dealt at bounce 1. The lists' lengths come from rt_host_tile_lists (wave_run.py writes them: one
//           word per tile, 0xFFFFFFFF for a tile that walks); such a block is charged a begin, a shade at 64 lanes, 60
//           for compaction and entry writes, 67 for the root passes and 20 per listed sphere on top of the block's own.
// Paths are the oracle's (make_ray / closest_sphere / scatter, oracle/rt_oracle.c); the tree is build_sphere_bvh's with
// its f32 boxes unpadded, as in packet_sim.cpp — a model of the kernel's padded fp16 test, not the test itself.
//
// It prints lane and wave counts of every block per round and per query, and an issue-slot price from rough weights
// (DESIGN.md §4 census: box step 37 VALU + 14 SALU, a walk call's entry ~50, a leaf sphere ~15 and a candidate's root
// ~45, an outer walk iteration's own bookkeeping ~12, begin ~130, shade ~260, a frame block ~340 and a pass of the
// dealing loop ~40). No latency, no issue arbitration.
//
// Build and run: python scripts/studies/wave_run.py [--hold 12] ...   (g++ -O2 -ffp-contract=off, see wave_run.py)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host/sphere_bvh.hpp"

extern "C" {
#include "../../oracle/rt_oracle.c"
}

static const hrt::SphereBvh* G;
static const float* GS;  // cx cy cz r2 per leaf sphere

static inline bool box_hit(const float* mn, const float* mx, v3 o, v3 inv, float bt, float& te) {
    float t0x = (mn[0] - o.x) * inv.x, t1x = (mx[0] - o.x) * inv.x;
    float t0y = (mn[1] - o.y) * inv.y, t1y = (mx[1] - o.y) * inv.y;
    float t0z = (mn[2] - o.z) * inv.z, t1z = (mx[2] - o.z) * inv.z;
    float tmin = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fmaxf(fminf(t0z, t1z), 0.0f));
    float tmax = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
    te = tmin;
    return tmin <= tmax && tmin <= bt;
}

struct Lane {
    bool have = false;
    int qs = 0;  // 0 start a query, 1 walking, 2 walk finished
    ray_t ray;
    uint32_t s = 0, bounce = 0;
    // the query (BvhQuery): next child word, stack, best t
    uint32_t node = 0, stack[64];
    int sp = 0;
    float bt = 0, a = 0;
    v3 inv;
    uint32_t cand = 0, cwaited = 0;  // the leaf's candidates not yet resolved (bit j: sphere first + j), iterations waited
};

struct Counts {  // w*: wave events, l*: lanes taking part
    double rounds = 0, queries = 0, samples = 0;
    double wblock = 0, wdeal = 0, ldeal = 0;
    double wbegin = 0, lbegin = 0;
    double wcall = 0, lcall = 0, wwalk = 0, lwalk = 0;
    double wbox = 0, lbox = 0, wleaf = 0, lleaf = 0, leaf_maxcnt = 0, leaf_maxcand = 0, whold = 0, lheld = 0;
    double wroot = 0, lroot = 0, wchold = 0, lcheld = 0;  // root-pass runs and their lanes (leaf_maxcand: their iterations)
    double wshade = 0, lshade = 0;
    double wres = 0, lres = 0, res_list = 0, res_surv = 0;  // blocks resolved when made: their rays, listed spheres, survivors
};

struct Sim {
    o_scene sc;
    uint32_t W, H, B, suspend_below, hold, job_frames, chold = 0, cwait = 0;
    bool blocktime = false;
    std::vector<uint32_t> list_len;  // per tile, 0xFFFFFFFF: walk
    Counts C;

    ray_t primary(uint32_t x, uint32_t y, uint32_t time, uint32_t& s) {  // fs_main prologue (oracle sample_pixel)
        s = (x * H + y) * time;
        float aspect = (float)W / (float)H;
        float r1 = rng_float(&s), r2 = rng_float(&s);
        float ssa = fmaf(r2, r2, r1 * r1), len = sqrtf(ssa);
        float px = ((float)x + 0.5f) + r1 / len, py = ((float)y + 0.5f) + r2 / len;
        float ux = (2.0f * (px / ((float)W - 1.0f)) - 1.0f) * aspect, uy = (2.0f * (py / ((float)H - 1.0f)) - 1.0f) * -1.0f;
        return make_ray(&sc, ux, uy, &s);
    }

    void begin(Lane& L) {  // bvh_begin: the large list, then the root
        const v3 o = L.ray.o, d = L.ray.d;
        L.a = dot3(d, d);
        float bt = FLT_MAX_REF;
        for (int k : G->large) {
            const o_sphere* sp = &sc.spheres[k];
            v3 oc = vsub(o, ld3(sp->center));
            float b = 2.0f * dot3(oc, d), c = dot3(oc, oc) - sp->radius * sp->radius;
            float disc = fmaf(b, b, -((4.0f * L.a) * c));
            if (disc < 0.0f) continue;
            float t = (-b - sqrtf(disc)) / (2.0f * L.a);
            if (t > 0.0f && t < bt) bt = t;
        }
        L.bt = bt;
        L.inv = V(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
        L.node = G->root_word;
        L.sp = 0;
        L.qs = 1;
    }

    // one box step of a lane; returns true when the lane wants another one (a hit child that is no leaf)
    bool box_step(Lane& L, bool& miss) {
        const hrt::SphereBvhNode& n = G->nodes[L.node];
        float tl, tr;
        const bool hl = box_hit(n.lmin, n.lmax, L.ray.o, L.inv, L.bt, tl), hr = box_hit(n.rmin, n.rmax, L.ray.o, L.inv, L.bt, tr);
        const bool lf = hl && (!hr || tl <= tr);
        if (hl && hr) L.stack[L.sp++] = lf ? n.right : n.left;
        miss = !(hl || hr);
        if (!miss) L.node = lf ? n.left : n.right;
        return !miss && !(L.node & hrt::BVH_LEAF_BIT);
    }

    // the leaf's first pass (sphere_candidate of every sphere: the lane's candidates) and its second (their roots)
    static void leaf_terms(const Lane& L, uint32_t j, float& b, float& disc) {
        const float* g = GS + 4 * (((L.node >> 4) & 0x07FFFFFFu) + j);
        v3 oc = V(L.ray.o.x - g[0], L.ray.o.y - g[1], L.ray.o.z - g[2]);
        b = 2.0f * dot3(oc, L.ray.d);
        disc = fmaf(b, b, -((4.0f * L.a) * (dot3(oc, oc) - g[3])));
    }
    uint32_t leaf_pass1(Lane& L) {
        const uint32_t cnt = L.node & 15u;
        L.cand = 0;
        for (uint32_t j = 0; j < cnt; j++) {
            float b, disc;
            leaf_terms(L, j, b, disc);
            if (disc >= 0.0f && b <= 0.0f) L.cand |= 1u << j;  // sphere_candidate
        }
        return cnt;
    }
    uint32_t leaf_roots(Lane& L) {
        const uint32_t n = (uint32_t)__builtin_popcount(L.cand);
        for (uint32_t j = 0; L.cand != 0; j++, L.cand >>= 1) {
            if (!(L.cand & 1u)) continue;
            float b, disc;
            leaf_terms(L, j, b, disc);
            float t = (-b - sqrtf(disc)) / (2.0f * L.a);
            if (t > 0.0f && t < L.bt) L.bt = t;
        }
        return n;
    }

    // bvh_walk_noovf for the lanes of `w` (qs == 1), in lockstep
    void walk(Lane* lanes, const std::vector<int>& w) {
        std::vector<int> act = w;  // lanes still in this call
        C.wcall++, C.lcall += act.size();
        std::vector<char> held(64), missed(64);
        while (!act.empty()) {
            C.wwalk++, C.lwalk += act.size();
            const uint32_t lim = std::min<uint32_t>(hold, (uint32_t)act.size());
            std::vector<int> D;
            for (int l : act) {
                held[l] = missed[l] = 0;
                if (!(lanes[l].node & hrt::BVH_LEAF_BIT)) D.push_back(l);
            }
            while (!D.empty()) {
                C.wbox++, C.lbox += D.size();
                std::vector<int> D2;
                for (int l : D) {
                    bool miss;
                    if (box_step(lanes[l], miss)) D2.push_back(l);
                    missed[l] = miss;
                }
                if (!D2.empty() && D2.size() < lim) {  // the descent hold
                    for (int l : D2) held[l] = 1;
                    C.whold++, C.lheld += D2.size();
                    break;
                }
                D.swap(D2);
            }
            // (a lane held with a candidate kept its leaf word only: it takes the first pass again)
            uint32_t nl = 0, mc = 0, mk = 0, nc = 0, waited = 0;
            for (int l : act) {
                if (held[l] || missed[l] || !(lanes[l].node & hrt::BVH_LEAF_BIT)) continue;
                if (lanes[l].cand == 0) lanes[l].cwaited = 0;
                nl++, mc = std::max(mc, leaf_pass1(lanes[l]));
                if (lanes[l].cand != 0) nc++, waited = std::max(waited, lanes[l].cwaited);
            }
            if (nl) C.wleaf++, C.lleaf += nl, C.leaf_maxcnt += mc;
            std::vector<char> cheld(64);
            if (nc && (nc >= chold || nc == act.size() || waited >= cwait)) {
                for (int l : act)
                    if (lanes[l].cand != 0) mk = std::max(mk, leaf_roots(lanes[l]));
                C.wroot++, C.lroot += nc, C.leaf_maxcand += mk;
            } else if (nc) {  // the candidate hold
                for (int l : act)
                    if (lanes[l].cand != 0) cheld[l] = 1, lanes[l].cwaited++;
                C.wchold++, C.lcheld += nc;
            }
            std::vector<int> next;
            for (int l : act) {
                Lane& L = lanes[l];
                if (!held[l] && !cheld[l]) {
                    if (L.sp == 0) {
                        L.qs = 2;
                        continue;
                    }
                    L.node = L.stack[--L.sp];
                }
                next.push_back(l);
            }
            act.swap(next);
            if (act.size() < suspend_below) break;  // suspended: the state stays in the lanes
        }
    }

    void shade(Lane& L) {
        C.queries++;
        hit_t h = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, FLT_MAX_REF, 0, 0};
        closest_sphere(&sc, L.ray, &h);
        bool done = true;
        if (!(fabsf(h.t - FLT_MAX_REF) < sc.eps)) {
            L.ray = scatter(&sc, &L.s, L.ray, &h);
            L.bounce++;
            done = L.bounce >= B;
        }
        if (done) L.have = false, C.samples++;
        L.qs = 0;
    }

    void wave(uint32_t njobs, uint32_t& seed) {
        Lane lanes[64];
        const uint32_t tw = (W + 7) / 8, th = (H + 7) / 8;
        uint32_t job = 0, job_tile = 0, job_f0 = 0, blk_f = 0, blk_next = 64, blk_cnt = 64;
        bool dealing = false, drained = false;
        struct Entry { ray_t r; uint32_t s; bool ok; uint32_t bounce; } blk[64];
        while (true) {
            // refill
            std::vector<int> need;
            for (int l = 0; l < 64; l++)
                if (!lanes[l].have && !drained) need.push_back(l);
            while (!need.empty()) {
                if (blk_next == blk_cnt) {
                    if (dealing && blk_f + 1 < job_frames) {
                        blk_f++;
                    } else {
                        if (job == njobs) {
                            drained = true;
                            break;
                        }
                        job++;
                        rng_int(&seed);
                        job_tile = seed % (tw * th);
                        rng_int(&seed);
                        job_f0 = seed % 1024u;
                        blk_f = 0;
                        dealing = true;
                    }
                    blk_next = 0;
                    C.wblock++;
                    for (int l = 0; l < 64; l++) {
                        const uint32_t x = (job_tile % tw) * 8 + (l & 7), y = (job_tile / tw) * 8 + (l >> 3);
                        blk[l].ok = x < W && y < H;
                        blk[l].bounce = 0;
                        if (blk[l].ok) blk[l].r = primary(x, y, 1000u + 10u * (job_f0 + blk_f), blk[l].s);
                    }
                    blk_cnt = 64;
                    if (blocktime && B >= 1 && list_len[job_tile] != 0xFFFFFFFFu) {
                        uint32_t n = 0, live = 0;
                        for (int l = 0; l < 64; l++) {
                            if (!blk[l].ok) continue;
                            live++, C.queries++;
                            hit_t h = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, FLT_MAX_REF, 0, 0};
                            closest_sphere(&sc, blk[l].r, &h);
                            if (fabsf(h.t - FLT_MAX_REF) < sc.eps || B == 1) {
                                C.samples++;
                                continue;
                            }
                            Entry e = blk[l];
                            e.r = scatter(&sc, &e.s, e.r, &h);
                            e.bounce = 1;
                            blk[n++] = e;  // (n <= l: compaction in place)
                        }
                        blk_cnt = n;
                        C.wres++, C.lres += live, C.res_list += list_len[job_tile], C.res_surv += n;
                    }
                }
                const uint32_t avail = blk_cnt - blk_next;
                C.wdeal++;
                std::vector<int> still;
                for (size_t rank = 0; rank < need.size(); rank++) {
                    Lane& L = lanes[need[rank]];
                    if (rank >= avail) {
                        still.push_back(need[rank]);
                        continue;
                    }
                    const Entry& e = blk[blk_next + rank];
                    if (!e.ok) continue;
                    L.ray = e.r, L.s = e.s, L.bounce = e.bounce, L.have = true, L.qs = 0;
                    C.ldeal++;
                }
                blk_next += std::min<uint32_t>((uint32_t)need.size(), avail);
                need.swap(still);
            }
            bool any = false;
            for (int l = 0; l < 64; l++) any |= lanes[l].have;
            if (!any) {
                if (drained) break;
                continue;  // (a block of a ragged tile gave nobody a sample)
            }
            C.rounds++;
            // begin
            uint32_t nb = 0;
            for (int l = 0; l < 64; l++) {
                Lane& L = lanes[l];
                if (!(L.have && L.qs == 0)) continue;
                if (L.bounce < B) begin(L), nb++;
                else L.qs = 3;
            }
            if (nb) C.wbegin++, C.lbegin += nb;
            // walk
            std::vector<int> w;
            for (int l = 0; l < 64; l++)
                if (lanes[l].have && lanes[l].qs == 1) w.push_back(l);
            if (!w.empty()) walk(lanes, w);
            // shade
            uint32_t ns = 0;
            for (int l = 0; l < 64; l++) {
                Lane& L = lanes[l];
                if (!(L.have && L.qs >= 2)) continue;
                ns++;
                if (L.qs == 2) shade(L);
                else L.have = false, L.qs = 0, C.samples++;
            }
            if (ns) C.wshade++, C.lshade += ns;
        }
    }
};

int main(int argc, char** argv) {
    if (argc < 9) {
        fprintf(stderr, "usage: wave_sim scene.bin W H bounces waves jobs_per_wave suspend_below hold [job_frames = 32] "
                        "[chold = 0] [cwait = 0] [blocktime = 0] [tile_list_lengths.bin]\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t nsl;
    float cam[20];
    if (fread(cam, 4, 20, f) != 20 || fread(&nsl, 4, 1, f) != 1) return 3;
    std::vector<o_sphere> sph(nsl);
    if (fread(sph.data(), sizeof(o_sphere), nsl, f) != nsl) return 3;
    fclose(f);
    Sim S;
    S.W = atoi(argv[2]), S.H = atoi(argv[3]), S.B = atoi(argv[4]);
    const uint32_t waves = atoi(argv[5]), jobs = atoi(argv[6]);
    S.suspend_below = std::max(atoi(argv[7]), 1), S.hold = atoi(argv[8]);
    S.job_frames = argc > 9 ? atoi(argv[9]) : 32;
    S.chold = argc > 10 ? atoi(argv[10]) : 0, S.cwait = argc > 11 ? atoi(argv[11]) : 0;
    S.blocktime = argc > 12 && atoi(argv[12]) != 0;
    if (S.blocktime) {
        const size_t nt = (size_t)((S.W + 7) / 8) * ((S.H + 7) / 8);
        S.list_len.resize(nt);
        FILE* lf = argc > 13 ? fopen(argv[13], "rb") : nullptr;
        if (!lf || fread(S.list_len.data(), 4, nt, lf) != nt) return 3;
        fclose(lf);
    }
    std::vector<float> cr(4 * nsl);
    for (uint32_t i = 0; i < nsl; i++) {
        cr[4 * i] = sph[i].center[0], cr[4 * i + 1] = sph[i].center[1], cr[4 * i + 2] = sph[i].center[2];
        cr[4 * i + 3] = sph[i].radius;
    }
    hrt::SphereBvh bvh = hrt::build_sphere_bvh(cr);
    G = &bvh;
    GS = bvh.sph.data();
    memset(&S.sc, 0, sizeof S.sc);
    S.sc.cam = (const o_camera*)cam;
    S.sc.k = tanf(S.sc.cam->params[2] * 0.5f);
    S.sc.spheres = sph.data();
    S.sc.nslots = nsl;
    S.sc.mode = MODE_SPHERE;
    S.sc.bounces = S.B;
    S.sc.eps = 1e-6f;
    S.sc.step_cap = 600;
    uint32_t seed = 12345u;
    for (uint32_t w = 0; w < waves; w++) S.wave(jobs, seed);
    const Counts& C = S.C;
    const double q = C.queries, q64 = q / 64.0, r = C.rounds;
    printf("suspend_below %u hold %u: %u waves x %u jobs x %u frames, %.0f samples, %.0f queries, %.0f rounds\n", S.suspend_below,
           S.hold, waves, jobs, S.job_frames, C.samples, q, r);
    printf("per round:  blocks %.4f  begin lanes %.2f  walk calls %.3f (lanes %.2f)  walk iterations %.3f  box steps %.3f  "
           "leaf steps %.3f  shade lanes %.2f\n",
           C.wblock / r, C.lbegin / r, C.wcall / r, C.lcall / std::max(C.wcall, 1.0), C.wwalk / r, C.wbox / r, C.wleaf / r,
           C.lshade / r);
    printf("per 64 queries (wave) / per query (lane):  refill blocks %.4f / deals %.3f  begin %.3f / %.3f  walk iterations %.3f / "
           "%.3f  box steps %.3f / %.3f  leaf steps %.3f / %.3f  shade %.3f / %.3f  rounds %.3f\n",
           C.wblock / q64, C.ldeal / q, C.wbegin / q64, C.lbegin / q, C.wwalk / q64, C.lwalk / q, C.wbox / q64, C.lbox / q,
           C.wleaf / q64, C.lleaf / q, C.wshade / q64, C.lshade / q, r / q64);
    printf("lanes per event:  walk iteration %.2f  box step %.2f  leaf step %.2f (max spheres %.2f, max candidates %.3f per leaf "
           "step)  shade %.2f  begin %.2f;  holds per 64 queries %.3f (lanes held %.2f)\n",
           C.lwalk / C.wwalk, C.lbox / C.wbox, C.lleaf / C.wleaf, C.leaf_maxcnt / C.wleaf, C.leaf_maxcand / C.wleaf,
           C.lshade / C.wshade, C.lbegin / std::max(C.wbegin, 1.0), C.whold / q64, C.lheld / std::max(C.whold, 1.0));
    printf("root pass per 64 queries:  runs %.2f  iterations %.2f  lanes per run %.1f;  candidate hold %u / %u: holds %.3f "
           "(lanes held %.2f)\n",
           C.wroot / q64, C.leaf_maxcand / q64, C.lroot / std::max(C.wroot, 1.0), S.chold, S.cwait, C.wchold / q64,
           C.lcheld / std::max(C.wchold, 1.0));
    // issue-slot price per query (rough weights, see the head of this file)
    // (a block resolved when made: its begin, shade, compaction, root passes and listed spheres, charged to the refill)
    const double c_res = (130.0 + 260.0 + 60.0 + 67.0) * C.wres + 20.0 * C.res_list;
    if (S.blocktime)
        printf("block time: %.0f of %.0f blocks resolved (%.1f rays, %.2f listed spheres, %.1f survivors each), %.3f of the "
               "queries\n",
               C.wres, C.wblock, C.lres / std::max(C.wres, 1.0), C.res_list / std::max(C.wres, 1.0),
               C.res_surv / std::max(C.wres, 1.0), C.lres / q);
    const double c_refill = 340.0 * C.wblock + 40.0 * C.wdeal + c_res, c_begin = 130.0 * C.wbegin, c_shade = 260.0 * C.wshade;
    const double c_walk = 51.0 * C.wbox + 50.0 * C.wcall + 15.0 * C.leaf_maxcnt + 45.0 * C.leaf_maxcand + 12.0 * C.wwalk;
    const double tot = c_refill + c_begin + c_walk + c_shade;
    printf("issue cost per query %.3f  shares: refill %.3f (block time %.3f of the total) begin %.3f walk %.3f shade %.3f\n",
           tot / q, c_refill / tot, c_res / tot, c_begin / tot, c_walk / tot, c_shade / tot);
    printf("JSON {\"suspend_below\": %u, \"hold\": %u, \"queries\": %.0f, \"walk_lanes\": %.3f, \"box_lanes\": %.3f, "
           "\"leaf_lanes\": %.3f, \"shade_lanes\": %.3f, \"wave_box_per_64q\": %.4f, \"lane_box_per_q\": %.4f, \"cost_per_query\": %.4f, "
           "\"share_refill\": %.4f, \"share_begin\": %.4f, \"share_walk\": %.4f, \"share_shade\": %.4f, \"chold\": %u, "
           "\"cwait\": %u, \"root_runs_per_64q\": %.4f, \"root_iterations_per_64q\": %.4f, \"root_lanes\": %.3f, \"blocktime\": %d, \"rounds_per_64q\": %.4f, "
           "\"share_blocktime\": %.4f}\n",
           S.suspend_below, S.hold, q, C.lwalk / C.wwalk, C.lbox / C.wbox, C.lleaf / C.wleaf, C.lshade / C.wshade, C.wbox / q64,
           C.lbox / q, tot / q, c_refill / tot, c_begin / tot, c_walk / tot, c_shade / tot, S.chold, S.cwait, C.wroot / q64,
           C.leaf_maxcand / q64, C.lroot / std::max(C.wroot, 1.0), (int)S.blocktime, r / q64, c_res / tot);
    return 0;
}
