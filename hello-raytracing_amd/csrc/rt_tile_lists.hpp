// rt_tile_lists.hpp — the per-tile primary candidate lists of the sphere program, as the host (renderer.cpp,
// rt_host_tile_lists) and the device (rt_kernels.hip k_tile_lists) both compile them: ONE rule, in f64 with +, -, *, /
// and sqrt alone (correctly rounded on both sides, no FMA: -ffp-contract=off), so the device lists equal the host
// mirror's byte for byte.
//
// A tile's list names every leaf sphere of the culling BVH (by BVH code) that a primary ray of the tile's 8x8 pixels
// could be accepted by, for any frame, jitter and lens sample; the large list is not listed (it is always tested). The
// kernels that use a list (k_trace_split's block-time resolve) test its spheres with the leaf's own arithmetic, so
// soundness is list >= what the walk could find, and a loose list costs tests, never bits.
//
// The hull of a tile's rays (make_ray, sphere mode): the pixel position is pixel + 0.5 + a jitter in [0, 1]^2; the
// rule covers pixel - 0.5 .. pixel + 2. The ray starts at eye + delta, |delta| <= |blur|, delta in world xy, and points
// at f = eye + F u, u the unit view direction of the pixel position and F its focus distance — make_ray normalises the
// view vector v with its fourth component, so F = focal |v.xyz| / |v.xyzw| <= focal, bounded over the tile as
// [F_lo, F_hi] (v is affine in the pixel position: its fourth component is extremal at the corners, |v.xyz| is at most
// its largest corner value and at least its central value less the largest corner distance). The ray's points are
//     eye + s u + (1 - s / F) delta,   s >= 0:
// the pinhole ray displaced by at most |1 - s / F| |blur|. The pinhole directions of a tile lie inside the cone
// around the tile's central direction through its four corner directions (the directions are a planar rectangle, the
// cone is convex); its half angle is widened by 0.1 % + 1e-6 rad, and by 8u (|eye| + F + |blur|) / (F - |blur|) for the
// f32 steps in which the kernels form the ray (f, the origin, f - origin), an error that grows with the eye's distance
// from the origin.
// A sphere (C, R) is listed unless the cone misses the ball (C, R + lens + pad):
//     lens = |blur| max |1 - s / F| over F in [F_lo, F_hi] and the s at which the ray can be within reach of the ball,
//     pad  = twice the culling walk's own bound on the distance by which a sphere accepted in f32 can miss
//            geometrically (DESIGN.md §Sphere BVH exactness), taken for this sphere: 8u R + min(16u D^2 / R, 2e-3 D) +
//            4u D + 8.1e-23 / F_lo, u = 2^-24, D a bound on the distance from a ray's origin to the ball's far side;
//            + 1e-6 D + 4u (|eye| + |blur|), the f32 origin's distance from the exact one.
// Degenerate inputs mark the tile "walk" (TILE_LIST_WALK: its blocks walk their primary rays as ever): a focal length
// <= 0 or |blur| >= F_lo / 2, a one-pixel-wide or -high image, the eye inside a
// leaf sphere's padded ball, a cone wider than 45 degrees, any value that is not finite, and a list longer than K.
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HRT_TILES_FN __host__ __device__ inline
#else
#define HRT_TILES_FN inline
#endif

namespace hrt_tiles {

constexpr uint32_t K_MAX = 8, WORDS = 1 + K_MAX, WALK = 0xFFFFFFFFu;  // (rt_device.hpp TILE_LIST_K, _WORDS, _WALK)

// What the rule reads: make_ray's constants as the kernels hold them (rt_device.hpp CamDev, f32), the image and the
// renderer's row share (KParams), and the leaf spheres in BVH order (cx, cy, cz, r * r).
struct View {
    float eye[4], dir[4], up[4], right[4];
    float focal, blur, k, aspect, wm1, hm1;
    uint32_t W, H;
    uint32_t row0, row_block, row_stride, nrows;  // local row kr is global row row0 + (kr / row_block) * row_stride + kr % row_block
    uint32_t tiles_w, tiles_h;
    uint32_t k_list;  // entries a list may hold (<= K_MAX)
};

HRT_TILES_FN bool fin64(double x) { return x - x == 0.0; }

// The tile's cone: central direction c (unit), sine and cosine of its widened half angle; false: the tile walks.
struct Cone {
    double c[3], sin_t, cos_t, f_lo, f_hi;
};
// the view vector of a pixel position: v[0..2], its length in v[4], the fourth component in v[3]; out = v.xyz / |v.xyz|
HRT_TILES_FN void view_dir(const View& V, double px, double py, double out[3], double v[5]) {
    const double ux = (2.0 * (px / (double)V.wm1) - 1.0) * (double)V.aspect;
    const double uy = -(2.0 * (py / (double)V.hm1) - 1.0);
    double l = 0.0;
    for (int i = 0; i < 4; i++) {
        v[i] = ((double)V.right[i] * ux) * (double)V.k + ((double)V.up[i] * uy) * (double)V.k + (double)V.dir[i];
        if (i < 3) l += v[i] * v[i];
    }
    l = sqrt(l);
    v[4] = l;
    for (int i = 0; i < 3; i++) out[i] = v[i] / l;
}
HRT_TILES_FN bool tile_cone(const View& V, uint32_t tile, Cone& T) {
    if (!((double)V.focal > 0.0) || !fin64((double)V.focal) || !fin64((double)V.blur)) return false;
    const double B = (double)V.blur < 0.0 ? -(double)V.blur : (double)V.blur;
    if (!((double)V.wm1 > 0.0) || !((double)V.hm1 > 0.0)) return false;
    const uint32_t tx = tile % V.tiles_w, ty = tile / V.tiles_w;
    const uint32_t x0 = tx * 8u, x1 = (x0 + 7u < V.W - 1u) ? x0 + 7u : V.W - 1u;
    if (x0 >= V.W) return false;
    // the tile's in-image local rows and the range of their global rows (a row share deals blocks of rows)
    const uint32_t k0 = ty * 8u;
    if (k0 >= V.nrows) return false;
    const uint32_t k1 = (k0 + 7u < V.nrows - 1u) ? k0 + 7u : V.nrows - 1u;
    uint32_t y0 = 0xFFFFFFFFu, y1 = 0u;
    for (uint32_t kr = k0; kr <= k1; kr++) {
        const uint32_t b = kr / V.row_block;
        const uint32_t y = V.row0 + b * V.row_stride + (kr - b * V.row_block);
        y0 = y < y0 ? y : y0;
        y1 = y > y1 ? y : y1;
    }
    const double pxa = (double)x0 - 0.5, pxb = (double)x1 + 2.0, pya = (double)y0 - 0.5, pyb = (double)y1 + 2.0;
    double vc[5];
    view_dir(V, 0.5 * (pxa + pxb), 0.5 * (pya + pyb), T.c, vc);
    double cmin = 1.0, w_lo = vc[3], w_hi = vc[3], m_hi = vc[4], far = 0.0;
    for (int i = 0; i < 4; i++) {
        double u[3], v[5];
        view_dir(V, (i & 1) ? pxb : pxa, (i & 2) ? pyb : pya, u, v);
        const double d = T.c[0] * u[0] + T.c[1] * u[1] + T.c[2] * u[2];
        if (!(d >= cmin)) cmin = d;  // (a NaN lands here and fails the test below)
        w_lo = v[3] < w_lo ? v[3] : w_lo;
        w_hi = v[3] > w_hi ? v[3] : w_hi;
        m_hi = v[4] > m_hi ? v[4] : m_hi;
        const double e[3] = {v[0] - vc[0], v[1] - vc[1], v[2] - vc[2]};
        const double el = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        far = el > far ? el : far;
    }
    if (!fin64(cmin) || !(cmin > 0.0)) return false;
    {
        // F = focal / sqrt(1 + q^2), q = |v.w| / |v.xyz| within [q_lo, q_hi]
        const double m_lo = vc[4] - far;
        if (!(m_lo > 0.0) || !fin64(m_hi) || !fin64(w_lo) || !fin64(w_hi)) return false;
        const double a_lo = w_lo < 0.0 ? -w_lo : w_lo, a_hi = w_hi < 0.0 ? -w_hi : w_hi;
        const double wmax = a_lo > a_hi ? a_lo : a_hi;
        const double wmin = (w_lo <= 0.0 && w_hi >= 0.0) ? 0.0 : (a_lo < a_hi ? a_lo : a_hi);
        const double q_hi = wmax / m_lo * 1.000001, q_lo = wmin / m_hi * 0.999999;
        T.f_lo = (double)V.focal / sqrt(1.0 + q_hi * q_hi) * 0.999999;
        T.f_hi = (double)V.focal / sqrt(1.0 + q_lo * q_lo) * 1.000001;
        if (!(T.f_lo > 0.0) || !fin64(T.f_hi) || !(B < 0.5 * T.f_lo)) return false;
    }
    // The kernels form the ray in f32: f = eye + vn * focal, o = eye + lens offset, d = f - o. Each component of f and o is
    // off by at most 2 * 2^-24 * (|eye| + F + B), so d is off by at most sqrt(3) * 4 * 2^-24 * (|eye| + F + B) < 8 u (..) in
    // length, against |d| >= F - B: the angle the cone is widened by on top of its own margin. It grows with the eye's
    // distance from the origin; a view where it reaches the pixel's angle fills its lists, and its tiles walk.
    const double E = sqrt((double)V.eye[0] * (double)V.eye[0] + (double)V.eye[1] * (double)V.eye[1] +
                          (double)V.eye[2] * (double)V.eye[2]);
    const double ray_ang = 8.0 * 0x1p-24 * (E + T.f_hi + B) / (T.f_lo - B);
    if (!fin64(ray_ang)) return false;
    const double s2 = 1.0 - cmin * cmin;
    const double st = sqrt(s2 > 0.0 ? s2 : 0.0) * 1.001 + 1e-6 + ray_ang;
    if (!(st < 0.7)) return false;
    T.sin_t = st;
    T.cos_t = sqrt(1.0 - st * st);
    return fin64(T.c[0]) && fin64(T.c[1]) && fin64(T.c[2]);
}

// 0: the cone misses the sphere's padded ball; 1: listed; 2: the tile walks (the eye inside the ball, or not finite).
HRT_TILES_FN int sphere_verdict(const View& V, const Cone& T, float cx, float cy, float cz, float rr) {
    const double u = 0x1p-24;
    const double B = (double)V.blur < 0.0 ? -(double)V.blur : (double)V.blur;
    const double w[3] = {(double)cx - (double)V.eye[0], (double)cy - (double)V.eye[1], (double)cz - (double)V.eye[2]};
    const double L = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double R = sqrt((double)rr);
    const double D = L + R + B;
    const double alt = 16.0 * u * (D * D) / R, lin = 2e-3 * D;
    // (twice the walk's own bound, bvh_slab_k's delta with its 4e-23 / |d| term at |d| >= F - B > F_lo / 2, and the f32
    // origin's distance from the exact one, tile_cone's bound: 4 u (|eye| + B))
    const double E = sqrt((double)V.eye[0] * (double)V.eye[0] + (double)V.eye[1] * (double)V.eye[1] +
                          (double)V.eye[2] * (double)V.eye[2]);
    const double pad = 2.0 * (8.0 * u * R + ((alt < lin) ? alt : lin) + 4.0 * u * D + 8.1e-23 / T.f_lo) + 1e-6 * D +
                       4.0 * u * (E + B);
    const double Rp = R + pad;
    const double smax = (L + Rp + B) / (1.0 - B / T.f_lo);
    double smin = L - Rp - B * (1.0 + smax / T.f_lo);
    smin = smin > 0.0 ? smin : 0.0;
    // (1 - s / F is monotone in s and in F: its largest magnitude is at a corner of [smin, smax] x [F_lo, F_hi])
    double em = 0.0;
    for (int i = 0; i < 4; i++) {
        double e = 1.0 - ((i & 1) ? smax : smin) / ((i & 2) ? T.f_hi : T.f_lo);
        e = e < 0.0 ? -e : e;
        em = e > em ? e : em;
    }
    const double Re = Rp + B * em;
    if (!fin64(Re) || !fin64(L) || !(L > Re * 1.000001)) return 2;
    const double sa = Re / L, ca = sqrt(1.0 - sa * sa);
    const double cs = T.cos_t * ca - T.sin_t * sa;  // cos(theta + alpha)
    if (!(cs > 0.0)) return 1;
    const double cp = (w[0] * T.c[0] + w[1] * T.c[1] + w[2] * T.c[2]) / L;
    return (cp < cs - 1e-12) ? 0 : 1;
}

// One tile's WORDS words: the count (or WALK) and the codes in ascending order, the rest zero.
// sph: the leaf spheres in BVH order, 4 floats each.
HRT_TILES_FN void tile_list(const View& V, uint32_t tile, const float* sph, uint32_t nleaf, uint32_t* out) {
    for (uint32_t i = 0; i < WORDS; i++) out[i] = 0u;
    Cone T;
    bool walk = !tile_cone(V, tile, T);
    uint32_t n = 0;
    for (uint32_t c = 0; c < nleaf && !walk; c++) {
        const int v = sphere_verdict(V, T, sph[4 * c], sph[4 * c + 1], sph[4 * c + 2], sph[4 * c + 3]);
        if (v == 2 || (v == 1 && n == V.k_list)) walk = true;
        else if (v == 1) out[1 + n++] = c;
    }
    if (walk) {
        for (uint32_t i = 1; i < WORDS; i++) out[i] = 0u;
        out[0] = WALK;
    } else {
        out[0] = n;
    }
}

}  // namespace hrt_tiles
