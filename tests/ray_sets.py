"""Seeded ray sets for the oracle-backed ray-query tests: the rays no camera makes.

scene_and_rays(name) gives a SceneDef and a RaySet of N_RAYS = 4099 rays (64 full waves and a ragged one) made from that
scene's own primitives (and, for heap scenes, its node boxes). Eight classes, half of every class aimed at a point of a
primitive and half not:
  a  axis-parallel: one or two components of d exactly +0 or -0, origins inside and outside the scene, and origins whose
     coordinate on the zero axis equals a node's bound, a vertex coordinate or a sphere's c_k, c_k +- r (0 * inf in the slabs)
  b  on the surface: origins at a first hit's point_on_ray (no offset) with the continuing, the scattered, an aimed and a
     random direction; origins exactly at a vertex and at a sphere's centre
  c  inside: in spheres (the ground sphere too), in the mesh, at the centre of the deepest node boxes
  d  length of d: a unit direction times 2^k, k in LENGTH_EXPONENTS, and directions with denormal components
  e  far origins: 1e3, 1e6 and 1e9 scene radii away
  f  grazing: impact parameter r (1 +- j 2^-23); through shared edges and vertices; in a triangle's plane with |det| on
     both sides of 1e-4; past an edge of a node's box, touching it in one point; through the world origin, where the
     zero-radius padding slots sit
  g  non-finite: NaN, +inf, -inf in one component of o or of d, and d = 0
  h  plain incoherent rays
Two layouts of the same rays: interleaved() mixes the classes in every wave, blocked() keeps whole waves of one class
(class d first, one length per wave), so the wave-uniform fallbacks run with 64 of 64 lanes out of range.

Importable without a GPU; the on-surface origins come from the CPU oracle's own first hits.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import hrt
import scenes
from hrt import Mesh, Sphere, Tree, Vec3

N_RAYS = 4099
CLASSES = "abcdefgh"
LENGTH_EXPONENTS = (-60, -40, -20, -12, 0, 12, 20, 40, 60)
NO_EXPONENT = 999
STEP_CAP = 600
_N_D = 640  # class d: ten kinds (nine lengths and the denormals) of one full wave each
_BIG = 50.0  # a sphere of at least this radius is ground, not a target to stand around


@dataclasses.dataclass
class RaySet:
    o: np.ndarray                # (N, 3) float32, interleaved order
    d: np.ndarray
    label: np.ndarray            # (N,) '<U1', the class of each ray
    length_exponent: np.ndarray  # (N,) int: k of a class-d ray of length 2^k, NO_EXPONENT otherwise

    def interleaved(self):
        return self.o, self.d, self.label

    def blocked(self):
        """(o, d, label, perm): ray i of this layout is ray perm[i] of the interleaved one. Class d first (its rays are
        kind-major, 64 per kind), then the other classes in order."""
        rank = np.array([0 if c == "d" else 1 + CLASSES.index(c) for c in self.label])
        perm = np.argsort(rank, kind="stable")
        return self.o[perm], self.d[perm], self.label[perm], perm


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


class _Scene:
    """The primitives of one scene, in float64, and the helpers the classes share."""

    def __init__(self, spheres, tris, nodes, first_hit, slots, seed):
        self.rng = np.random.default_rng(seed)
        self.first_hit = first_hit
        self.slots = slots
        self.c = self.r = None
        self.va = self.vb = self.vc = None
        if spheres is not None and len(spheres):
            self.c = spheres["center"].astype(np.float64)
            self.r = spheres["radius"].astype(np.float64)
        if tris is not None and len(tris):
            self.va, self.vb, self.vc = (tris[k][:, :3].astype(np.float64) for k in ("a", "b", "c"))
        self.boxes = None
        if nodes is not None and len(nodes) > 1:
            lo, hi = nodes["bound_min"][1:, :3].astype(np.float64), nodes["bound_max"][1:, :3].astype(np.float64)
            ok = np.isfinite(lo).all(1) & np.isfinite(hi).all(1) & (lo <= hi).all(1)
            if ok.any():
                self.boxes = (lo[ok], hi[ok], np.flatnonzero(ok) + 1)
        self.small = np.flatnonzero(self.r < _BIG) if self.c is not None else np.zeros(0, int)
        cents = []
        if len(self.small):
            cents.append(self.c[self.small])
        if self.va is not None:
            cents.append((self.va + self.vb + self.vc) / 3.0)
        cents = np.concatenate(cents)
        self.centre = np.median(cents, axis=0)
        dist = np.linalg.norm(cents - self.centre, axis=1)
        self.R = max(float(np.percentile(dist, 90)), 1.0)
        # the side of the scene its ground does not hide: away from a ground sphere, or off a floor (a triangle far larger
        # than the others), so that rays which are to miss can be sent where there is sky
        self.up = None
        if self.c is not None and (self.r >= _BIG).any():
            g = int(np.argmax(self.r))
            self.up = (self.centre - self.c[g]) / np.linalg.norm(self.centre - self.c[g])
        elif self.va is not None:
            nrm = np.cross(self.vb - self.va, self.vc - self.va)
            area = np.linalg.norm(nrm, axis=1)
            g = int(np.argmax(area))
            if area[g] > 20.0 * np.median(area):
                up = nrm[g] / area[g]
                self.up = up if (self.centre - self.va[g]) @ up >= 0.0 else -up

    def skyward(self, v):
        """v mirrored into the half-space the ground does not hide (rows of an (n, 3) array, or one vector)."""
        if self.up is None:
            return v
        return v - 2.0 * np.minimum(v @ self.up, 0.0)[..., None] * self.up

    # ---- points of primitives
    def sphere_points(self, n, which=None):
        rng = self.rng
        k = self.small[rng.integers(0, len(self.small), n)] if which is None else which
        return self.c[k] + self.r[k, None] * _unit(rng, n) * rng.uniform(0.0, 0.9, (n, 1)), k

    def tri_points(self, n, which=None):
        rng = self.rng
        k = rng.integers(0, len(self.va), n) if which is None else which
        w = rng.dirichlet((2.0, 2.0, 2.0), n)
        return w[:, :1] * self.va[k] + w[:, 1:2] * self.vb[k] + w[:, 2:] * self.vc[k], k

    def points(self, n):
        """n points of primitives (inside small spheres, inside triangles): the things to aim at."""
        have_s, have_t = len(self.small) > 0, self.va is not None
        if have_s and have_t:
            ps, pt = self.sphere_points(n)[0], self.tri_points(n)[0]
            return np.where((np.arange(n) % 2 == 0)[:, None], ps, pt)
        return self.sphere_points(n)[0] if have_s else self.tri_points(n)[0]

    def off_points(self, n):
        """n points in a box 3 R around the scene: what the rays that are not aimed at a primitive go through."""
        return self.centre + self.R * self.rng.uniform(-3.0, 3.0, (n, 3))

    def outside(self, n, lo=1.5, hi=4.0):
        return self.centre + self.R * self.rng.uniform(lo, hi, (n, 1)) * _unit(self.rng, n)

    def targets(self, n):
        """Aimed for even j, not aimed for odd j."""
        return np.where((np.arange(n) % 2 == 0)[:, None], self.points(n), self.off_points(n))

    def scale(self, d):
        """The sphere program does not normalise d: any length. The triangle programs' camera rays are unit vectors; keep
        the callers' rays near that (the thresholds on |det| and t are absolute), class d aside."""
        n = len(d)
        if self.va is None:
            return d * self.rng.uniform(0.25, 4.0, (n, 1))
        return d / np.linalg.norm(d, axis=1, keepdims=True) * self.rng.uniform(0.8, 1.25, (n, 1))

    # ---- a
    def class_a(self, n):
        rng = self.rng
        j = np.arange(n)
        kind = (j // 2) % 3  # origin: 0 inside the scene, 1 outside, 2 with o_k on a plane of the scene
        k0 = rng.integers(0, 3, n)
        two = rng.integers(0, 2, n) == 1
        k1 = (k0 + 1 + rng.integers(0, 2, n)) % 3
        p = self.targets(n)
        snap = np.flatnonzero(kind == 2)
        p[snap] = self._plane_points(snap, k0[snap], p[snap])
        d = rng.uniform(0.1, 1.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
        d = self.scale(d)
        d[j, k0] = rng.choice([0.0, -0.0], n)
        z1 = rng.choice([0.0, -0.0], n)
        d[j[two], k1[two]] = z1[two]
        s = np.where(kind == 1, rng.uniform(2.0, 4.0, n), rng.uniform(0.05, 0.5, n)) * self.R
        s = s / np.linalg.norm(d, axis=1)
        p32 = p.astype(np.float32).astype(np.float64)
        o = p32 - d * s[:, None]
        o[j, k0] = p32[j, k0]  # (o_k = p_k - (+-0) s: the plane's own f32 coordinate)
        return o, d

    def _plane_points(self, idx, k0, p):
        """For the rays idx (zero axis k0, target p): a target whose k0 coordinate is exactly a coordinate of the scene.
        Aimed rays (even index) get a point of a primitive in such a plane: a triangle's middle vertex on that axis and a
        point of the segment the plane cuts out of the triangle, or a sphere's centre plane or tangent plane. The others
        get a node's bound, a vertex coordinate or c_k +- r."""
        rng = self.rng
        p = p.copy()
        for q, (i, k) in enumerate(zip(idx, k0)):
            aimed = i % 2 == 0
            use_tri = self.va is not None and (len(self.small) == 0 or (i // 2) % 2 == 0)
            if aimed and use_tri:
                t = rng.integers(0, len(self.va))
                v = np.stack([self.va[t], self.vb[t], self.vc[t]])
                order = np.argsort(v[:, k])
                lo, mid, hi = v[order[0]], v[order[1]], v[order[2]]
                span = hi[k] - lo[k]
                far = lo + (hi - lo) * ((mid[k] - lo[k]) / span) if span > 0 else hi
                p[q] = mid + (far - mid) * rng.uniform(0.0, 0.9)
                p[q, k] = mid[k]
            elif aimed:
                s = self.small[rng.integers(0, len(self.small))]
                u = _unit(rng, 1)[0] * rng.uniform(0.0, 0.9)
                p[q] = self.c[s] + self.r[s] * u
                p[q, k] = self.c[s, k] + self.r[s] * (0.0, 0.0, 1.0, -1.0)[(i // 4) % 4]
            elif self.boxes is not None and (i // 2) % 2 == 0:
                b = rng.integers(0, len(self.boxes[0]))
                p[q, k] = self.boxes[(i // 4) % 2][b, k]
            elif self.va is not None and (len(self.small) == 0 or (i // 4) % 2 == 0):
                t = rng.integers(0, len(self.va))
                p[q, k] = (self.va, self.vb, self.vc)[rng.integers(0, 3)][t, k]
            else:
                s = self.small[rng.integers(0, len(self.small))]
                p[q, k] = self.c[s, k] + self.r[s] * (0.0, 1.0, -1.0)[(i // 8) % 3]
        return p

    # ---- b
    def class_b(self, n):
        rng = self.rng
        m = 4 * n
        so = self.outside(m, 1.2, 3.0)
        sd = self.scale(self.points(m) - so)
        hit, hp, hd = self.first_hit(so.astype(np.float32), sd.astype(np.float32))
        ok = np.flatnonzero(hit & np.isfinite(hp).all(1) & np.isfinite(hd).all(1))
        assert len(ok) >= 8, "the scene's seed rays hit nothing"
        pick = ok[np.arange(n) % len(ok)]
        o = hp[pick].astype(np.float64)
        j = np.arange(n)
        kind = (j // 2) % 5
        aimed = j % 2 == 0
        cont = sd.astype(np.float32).astype(np.float64)[pick]
        scat = hd[pick].astype(np.float64)
        to_point = self.scale(self.points(n) - o)
        rand = self.scale(_unit(rng, n))
        # kinds 0, 1: the continuing and the scattered direction (even j) against a random one (odd j) from the same kind
        # of origin; kind 2, 3: aimed / random; kind 4: from a vertex or a sphere's centre, aimed / random
        d = np.where(aimed[:, None], to_point, rand)
        d[(kind == 0) & aimed] = cont[(kind == 0) & aimed]
        d[(kind == 1) & aimed] = scat[(kind == 1) & aimed]
        at = np.flatnonzero(kind == 4)
        for q in at:
            if self.va is not None and (len(self.small) == 0 or (q // 10) % 2 == 0):
                o[q] = (self.va, self.vb, self.vc)[rng.integers(0, 3)][rng.integers(0, len(self.va))]
            else:
                o[q] = self.c[rng.integers(0, len(self.c))]
        d[at] = np.where(aimed[at, None], self.scale(self.points(len(at)) - o[at]), rand[at])
        return o, d

    # ---- c
    def class_c(self, n):
        rng = self.rng
        o = np.zeros((n, 3))
        outward = np.zeros(n, bool)
        for q in range(n):
            kind = (q // 2) % 4
            if self.c is None:  # triangles only: inside the mesh (a third) and inside the deepest boxes
                kind = 2 if (q // 2) % 3 == 0 else 3
            if kind in (0, 1) and self.c is not None:
                s = rng.integers(0, len(self.c)) if kind == 0 else int(np.argmax(self.r))
                if self.r[s] >= _BIG:  # the ground: just under the surface, below the scene
                    u = self.centre + self.R * rng.uniform(-1.0, 1.0, 3) - self.c[s]
                    u /= np.linalg.norm(u)
                    o[q] = self.c[s] + self.r[s] * (1.0 - rng.uniform(1e-4, 2e-2)) * u
                else:
                    o[q] = self.c[s] + self.r[s] * rng.uniform(0.0, 0.95) * _unit(rng, 1)[0]
            elif kind == 3 and self.boxes is not None:  # the centre of one of the deepest boxes
                lo, hi, idx = self.boxes
                deep = np.flatnonzero(idx >= idx.max() // 2)
                b = deep[rng.integers(0, len(deep))]
                o[q] = 0.5 * (lo[b] + hi[b])
                if q % 2 == 1:  # not aimed: in the box's outer corner, heading out, so a box at the mesh's skin has a way out
                    o[q] += 0.45 * (hi[b] - lo[b]) * np.sign(o[q] - self.centre)
                    outward[q] = True
            elif self.va is not None:  # inside the mesh: from a point of a triangle a little towards the middle
                pt = self.tri_points(1)[0][0]
                o[q] = pt + (self.centre - pt) * rng.uniform(0.02, 0.6)
            else:
                s = self.small[rng.integers(0, len(self.small))]
                o[q] = self.c[s] + self.r[s] * rng.uniform(0.0, 0.95) * _unit(rng, 1)[0]
        aimed = (np.arange(n) % 2 == 0)[:, None]
        away = self.skyward(o - self.centre + 0.3 * self.R * _unit(rng, n))
        d = self.scale(np.where(aimed, self.points(n) - o, np.where(outward[:, None], away, _unit(rng, n))))
        return o, d

    # ---- d
    def class_d(self, n):
        """Kind-major: rays 64 q .. 64 q + 63 have length 2^LENGTH_EXPONENTS[q]; the last kind has denormal components.
        Aimed rays start close to their target (within a few radii or edge lengths), so that b * b of the sphere test
        stays finite at 2^60."""
        rng = self.rng
        per = n // 10
        tgt = self.points(n)
        near = tgt + rng.uniform(0.8, 2.5, (n, 1)) * _unit(rng, n)
        o = np.where((np.arange(n) % 2 == 0)[:, None], near, self.outside(n, 0.5, 2.0))
        u = np.where((np.arange(n) % 2 == 0)[:, None], tgt - o, _unit(rng, n))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        kinds = np.minimum(np.arange(n) // per, 9)
        d = u.astype(np.float32)
        expo = np.full(n, NO_EXPONENT)
        for q, k in enumerate(LENGTH_EXPONENTS):
            m = kinds == q
            d[m] = d[m] * np.float32(2.0 ** k)  # (exact)
            expo[m] = k
        den = np.flatnonzero(kinds == 9)
        tiny = np.array([1e-40, -3e-42, 1.4e-45, -1e-39, 5e-41], np.float32)
        for q in den:
            form = (q // 2) % 3
            if form == 0:    # one denormal component
                d[q, rng.integers(0, 3)] = tiny[q % 5]
            elif form == 1:  # two
                k = rng.integers(0, 3)
                d[q, k], d[q, (k + 1) % 3] = tiny[q % 5], tiny[(q + 2) % 5]
            else:            # the whole direction scaled into the denormals
                d[q] = d[q] * np.float32(2.0 ** -130)
        return o, d, expo

    # ---- e
    def class_e(self, n):
        rng = self.rng
        j = np.arange(n)
        far = np.array([1e3, 1e3, 1e6, 1e9])[(j // 2) % 4]
        p = self.targets(n)
        if self.c is not None and (self.r >= _BIG).any():  # a quarter of the aimed rays: the ground below the scene
            g = int(np.argmax(self.r))
            m = np.flatnonzero((j % 8) == 0)
            u = self.centre + self.R * rng.uniform(-1.0, 1.0, (len(m), 3)) - self.c[g]
            p[m] = self.c[g] + self.r[g] * u / np.linalg.norm(u, axis=1, keepdims=True)
        u = self.skyward(_unit(rng, n))
        o = self.centre + (self.R * far)[:, None] * u
        # every other ray that is not aimed passes the whole scene, the ground included, at 0.3 of its distance
        wide = np.flatnonzero(j % 4 == 1)
        side = np.cross(u[wide], _unit(rng, len(wide)))
        p[wide] = self.centre + 0.3 * (self.R * far[wide])[:, None] * side / np.linalg.norm(side, axis=1, keepdims=True)
        d = p - o
        unitd = d / np.linalg.norm(d, axis=1, keepdims=True)
        d = np.where(((j // 8) % 2 == 0)[:, None] | (self.va is not None), unitd, d)
        return o, d

    # ---- f
    def class_f(self, n):
        rng = self.rng
        o, d = np.zeros((n, 3)), np.zeros((n, 3))
        forms = []
        if len(self.small):
            forms.append("sphere")
        if self.va is not None:
            forms += ["edge", "vertex", "plane"]
        if self.boxes is not None:
            forms += ["box", "box"]
        forms.append("origin")
        for q in range(n):
            form = forms[(q // 2) % len(forms)]
            aimed = q % 2 == 0
            w = _unit(rng, 1)[0]
            back = self.R * rng.uniform(0.3, 3.0)
            if not aimed:  # (past the thing it grazes into the sky)
                w = self.skyward(w)
            if form == "sphere":
                s = self.small[rng.integers(0, len(self.small))]
                jj = (q // (2 * len(forms))) % 9
                # aimed: inside by j ulps (j = 0: exactly r); not aimed: outside by j + 1
                b = self.r[s] * (1.0 - jj * 2.0 ** -23 if aimed else 1.0 + (jj + 1) * 2.0 ** -23)
                u = np.cross(w, _unit(rng, 1)[0])
                u /= np.linalg.norm(u)
                o[q], d[q] = self.c[s] + u * b - w * back, w
            elif form in ("edge", "vertex"):
                t = rng.integers(0, len(self.va))
                v = (self.va[t], self.vb[t], self.vc[t])
                e = rng.integers(0, 3)
                pt = v[e] if form == "vertex" else v[e] + (v[(e + 1) % 3] - v[e]) * rng.uniform(0.05, 0.95)
                if not aimed:  # past the edge or vertex, outside this triangle, by a few ulps of the point
                    out = pt - (v[0] + v[1] + v[2]) / 3.0
                    pt = pt + out / max(np.linalg.norm(out), 1e-30) * np.abs(pt).max() * rng.integers(1, 6) * 2.0 ** -22
                o[q], d[q] = pt - w * back, w
            elif form == "box":
                # past an edge of a node's box (the root's half the time), touching it there and nowhere else: along the
                # edge's axis k anything, across it (+, -), so both other slabs meet in one point; not aimed: a few ulps out
                lo, hi, idx = self.boxes
                b = 0 if not aimed or (q // (2 * len(forms))) % 2 == 0 else rng.integers(0, len(lo))
                k = rng.integers(0, 3)
                k1, k2 = (k + 1) % 3, (k + 2) % 3
                pt = lo[b] + (hi[b] - lo[b]) * rng.uniform(0.0, 1.0, 3)
                s1, s2 = rng.choice([-1.0, 1.0], 2)
                pt[k1] = hi[b, k1] if s1 > 0 else lo[b, k1]
                pt[k2] = hi[b, k2] if s2 > 0 else lo[b, k2]
                w = np.zeros(3)
                w[k], w[k1], w[k2] = rng.uniform(-1, 1), s1 * rng.uniform(0.2, 1), -s2 * rng.uniform(0.2, 1)
                w /= np.linalg.norm(w)
                if not aimed:
                    ulps = np.abs(pt).max() * rng.integers(1, 6) * 2.0 ** -22
                    pt[k1] += s1 * ulps
                    pt[k2] += s2 * ulps
                o[q], d[q] = pt - w * back, w
            elif form == "plane":
                t = rng.integers(0, len(self.va))
                e1, e2 = self.vb[t] - self.va[t], self.vc[t] - self.va[t]
                N = np.cross(e1, e2)
                area2 = np.linalg.norm(N)
                if area2 == 0.0:
                    o[q], d[q] = self.off_points(1)[0], w
                    continue
                g = e1 * rng.uniform(-1, 1) + e2 * rng.uniform(-1, 1)
                g /= max(np.linalg.norm(g), 1e-30)
                # aimed: |det| = |d . N| just above 1e-4; not aimed: just below
                det = 1e-4 * (1.0 + rng.uniform(1e-4, 1e-1)) if aimed else 1e-4 * (1.0 - rng.uniform(1e-4, 1e-1))
                dd = g + N / area2 * (det / area2) * rng.choice([-1.0, 1.0])
                pt = self.tri_points(1, np.array([t]))[0][0]
                back = min(back, 2.0)
                o[q], d[q] = pt - dd * back, dd
            else:  # through the world origin: d = -o exactly, so the discriminant of a zero-radius slot there is rounding
                if aimed:
                    oo = (w * rng.uniform(0.2, 0.9) * max(np.linalg.norm(self.centre), 1.0)).astype(np.float32)
                    o[q], d[q] = oo, -oo.astype(np.float64) * 2.0 ** rng.integers(-2, 3)
                else:
                    o[q], d[q] = w * back, -w + 1e-3 * _unit(rng, 1)[0]
        scaled = self.scale(d)
        keep = np.array([forms[(q // 2) % len(forms)] in ("plane", "origin") for q in range(n)])
        return o, np.where(keep[:, None], d, scaled)

    # ---- g
    def class_g(self, n):
        rng = self.rng
        o = self.outside(n)
        d = self.scale(self.targets(n) - o)
        o, d = o.astype(np.float32), d.astype(np.float32)
        bad = (np.nan, np.inf, -np.inf)
        for q in range(n):
            form = (q // 2) % 7
            if form == 6:
                d[q] = (0.0, -0.0)[(q // 14) % 2]
            else:
                (o if form < 3 else d)[q, rng.integers(0, 3)] = bad[form % 3]
        return o, d

    # ---- h
    def class_h(self, n):
        rng = self.rng
        o = np.where((np.arange(n) % 4 < 2)[:, None], self.outside(n), self.off_points(n))
        d = self.scale(np.where((np.arange(n) % 2 == 0)[:, None], self.points(n) - o, _unit(rng, n)))
        return o, d


def make_rays(spheres, tris, nodes, first_hit, slots: int = 0, seed: int = 20261021) -> RaySet:
    """The ray set of one scene. spheres: SPHERE_DTYPE or None; tris, nodes: TRIANGLE_DTYPE / NODE_DTYPE of a heap, or
    None; first_hit(o, d) -> (hit mask, point_on_ray float32, scattered direction float32): the oracle's."""
    sc = _Scene(spheres, tris, nodes, first_hit, slots, seed)
    rest = N_RAYS - _N_D
    sizes = {c: rest // 7 for c in CLASSES if c != "d"}
    sizes["d"] = _N_D
    sizes["h"] += rest - 7 * (rest // 7)
    parts, expo = {}, {}
    with np.errstate(all="ignore"):
        for c in CLASSES:
            out = getattr(sc, "class_" + c)(sizes[c])
            parts[c] = (np.asarray(out[0], np.float32), np.asarray(out[1], np.float32))
            expo[c] = out[2] if len(out) > 2 else np.full(sizes[c], NO_EXPONENT)
    o = np.concatenate([parts[c][0] for c in CLASSES])
    d = np.concatenate([parts[c][1] for c in CLASSES])
    label = np.concatenate([np.full(sizes[c], c) for c in CLASSES])
    ex = np.concatenate([expo[c] for c in CLASSES])
    frac = np.concatenate([(np.arange(sizes[c]) + 0.5) / sizes[c] for c in CLASSES])
    order = np.argsort(frac, kind="stable")  # every class spread evenly over the whole set
    return RaySet(np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order]), label[order], ex[order])


# ------------------------------------------------------------------------------------------------ the scenes
def _tiny_heap(k):
    """k triangles (1, 2 or 3) that face each other across a gap, over a ground sphere with a small sphere beside them:
    a mixed scene, so that rays that start on the one triangle still have something to hit."""
    import test_gpu_cast_rays as cast

    quads = [((-1.0, 0.0, -5.0), (1.0, 0.0, -5.0), (0.0, 1.6, -5.2)),
             ((-1.0, 0.1, -3.6), (0.0, 1.5, -3.5), (1.0, 0.2, -3.4)),
             ((-1.2, 0.0, -4.9), (-1.1, 1.4, -4.2), (-1.3, 0.1, -3.5))][:k]
    total = k + 2
    tree = Tree()
    for i, tri in enumerate(quads):
        obj = "".join("v %.9g %.9g %.9g\n" % v for v in tri) + "f 1 2 3\n"
        tree.add_mesh(Mesh.load_obj(obj.encode(), cast._material(2 + i, total)))
    tree.build()
    sp = hrt.spheres_array([Sphere._make(Vec3(0.0, -100.5, -4.5), 100.0, cast._material(0, total)),
                            Sphere._make(Vec3(1.6, 0.3, -4.4), 0.6, cast._material(1, total))])
    cam = scenes.config_c4(8, 8, 1).camera
    return scenes.SceneDef(f"heap{k}", hrt.RT_MODE_MIXED, 64, 40, cam, sp, bvh=tree.view(), min_sphere_slots=0)


def _coincident():
    """Spheres that share centre and radius with another slot (pairs, and one triple), each with its own material, over
    a ground sphere: the lower slot wins."""
    import test_gpu_cast_rays as cast

    base = [((1.4 * i, 0.9 * j, -6.0 - 0.3 * i), 0.45 + 0.02 * j) for i in range(-2, 3) for j in range(-1, 2)]
    every = base + base[:12] + base[:1] + [((0.0, -1004.0, -6.0), 1000.0)]
    sp = hrt.spheres_array([Sphere._make(Vec3(*c), r, cast._material(k, len(every))) for k, (c, r) in enumerate(every)])
    cam = cast.grid_scene(8, 8).camera
    return scenes.SceneDef("coincident", hrt.RT_MODE_SPHERE, 64, 40, cam, sp, min_sphere_slots=0)


def _rtiow():
    sd = scenes.config_c3(64, 40, 1)
    sd.bounces = None
    return sd


def _own_bounces(sd):
    """The reference's bounce cap of the scene's program (10 sphere, 5 triangle and mixed) instead of the builders' 1."""
    return dataclasses.replace(sd, bounces=None)


def _cast(name, *a):
    import test_gpu_cast_rays as cast

    return _own_bounces(getattr(cast, name)(64, 40, *a))


SCENES = {
    "grid": lambda: _cast("grid_scene", 0),
    "grid-100": lambda: _cast("grid_scene", 100),
    "cube": lambda: _cast("cube_scene"),
    "suzane": lambda: _cast("suzane_scene"),
    "mixed-simple": lambda: _cast("mixed_scene", 0),
    "mixed-defer": lambda: _cast("mixed_scene", 12),
    "mixed-bvh": lambda: _cast("mixed_scene", 60),
    "dragon": lambda: _cast("dragon_scene"),
    "rtiow": _rtiow,
    "coincident": _coincident,
    "heap1": lambda: _tiny_heap(1),
    "heap2": lambda: _tiny_heap(2),
    "heap3": lambda: _tiny_heap(3),
}


@functools.lru_cache(maxsize=None)
def scene_and_rays(name: str):
    """(SceneDef, RaySet) of one of SCENES; made once per process."""
    sd = SCENES[name]()

    def first_hit(o, d):
        no, nd, _, _, _, hit = scenes.oracle_bounce_step(sd, o, d, np.arange(1, len(o) + 1, dtype=np.uint32),
                                                         np.ones_like(o), step_cap=STEP_CAP)
        return hit, no, nd

    spheres = sd.spheres if sd.mode != hrt.RT_MODE_TRIS else None
    tris = nodes = None
    if sd.mode != hrt.RT_MODE_SPHERE:
        nodes, tris = sd.bvh[1], sd.bvh[2]
    slots = sd.min_sphere_slots if sd.min_sphere_slots is not None else (100 if sd.mode == hrt.RT_MODE_SPHERE else 0)
    return sd, make_rays(spheres, tris, nodes, first_hit, slots=slots)
