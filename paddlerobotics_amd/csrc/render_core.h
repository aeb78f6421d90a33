// render_core.h -- the camera renderer behind etg_render (include/etgsim_render.h): one robot on its own terrain per image.
//
// Everything here is ETG_HD, so the same source runs in the gfx950 kernel (etg_render.hip) and, compiled for the host, in the
// test-only shim (tests/render_emu).  Per image:
//   build_prims   the 17 primitives from a state row [37] (pos3, quat4 xyzw, ..., q12 at column 13) with the physics tick's own leg
//                 formulas (etg_core16.h: leg_geometry): trunk box, per leg a hip sphere at o1, a thigh capsule o2 -> o3, a calf
//                 capsule o3 -> pf and the foot sphere at pf, plus a bounding sphere around all of them
//   make_camera   the camera inverse of a pybullet view / projection matrix pair (column-major, gluLookAt / gluPerspective)
//   shade_pixel   one ray through the pixel centre: robot primitives (skipped when the ray misses the bounding sphere) and the
//                 terrain (plane z = 0, or the robot's heightfield band marched one cell per step and refined by bisection), then
//                 albedo x (ambient + diffuse max(0, n.L)) with one shadow ray toward L against the robot's primitives
// fp32 throughout; no infinities are formed (the library is built with -ffinite-math-only): "no hit" is a large finite t.
#pragma once

#include "etg_layout.h"

namespace etg {
namespace render {

// ---- the renderer's constants: one table ---------------------------------------------------------------------------------------
constexpr float kHipRadius = 0.04f;      // m, hip sphere at o1 (visual only: the physics has no hip collider)
constexpr float kThighRadius = 0.022f;   // m, thigh capsule o2 -> o3 (visual)
constexpr float kCalfRadius = 0.013f;    // m, calf capsule o3 -> pf (visual; the foot sphere is the collision radius)
constexpr float kDrawDist = 20.0f;       // m from the camera: terrain farther away is sky
constexpr float kChecker = 0.5f;         // m, side of a ground checkerboard square (world x, y)
constexpr int kBisect = 16;              // bisection steps that refine a heightfield hit inside one march step
constexpr int kMaxMarch = 4096;          // march steps at most per ray (longer spans take longer steps)
constexpr float kShadowLift = 2e-4f;     // m, a shadow ray starts this far out along the surface normal
constexpr float kSlabMargin = 1e-3f;     // m, the march's height slab is widened by this: a ray that meets terrain at exactly the
                                         // lowest height still sees the crossing under fp32 rounding
constexpr float kFar = 1e30f;            // "no hit"
// light: a unit direction TOWARD the light (from above, in front of and left of a robot walking along +x)
constexpr float kLightX = 0.36f, kLightY = 0.48f, kLightZ = 0.80f;
constexpr float kAmbient = 0.35f, kDiffuse = 0.65f;
// albedos (linear, 0..1) and the sky colour
constexpr float kSkyR = 0.62f, kSkyG = 0.76f, kSkyB = 0.92f;
constexpr float kGroundA = 0.58f, kGroundB = 0.42f;                          // checkerboard greys
constexpr float kTrunkR = 0.85f, kTrunkG = 0.55f, kTrunkB = 0.20f;
constexpr float kHipR = 0.25f, kHipG = 0.25f, kHipB = 0.28f;
constexpr float kThighR = 0.80f, kThighG = 0.80f, kThighB = 0.82f;
constexpr float kCalfR = 0.30f, kCalfG = 0.30f, kCalfB = 0.34f;
constexpr float kFootR = 0.10f, kFootG = 0.10f, kFootB = 0.10f;

// segmentation ids (the seg output): -1 sky, 0 terrain, 1 trunk, 2 + 4 leg + part
enum { SEG_SKY = -1, SEG_TERRAIN = 0, SEG_TRUNK = 1, SEG_LEG0 = 2 };
enum { PART_HIP = 0, PART_THIGH = 1, PART_CALF = 2, PART_FOOT = 3 };

// the handle's constants a render reads (a plain kernel argument)
struct RenderScene {
  const float* hf;                 // heights [bands][ny][nx] (terrain == 1), device (kernel) or host (shim) memory
  int terrain, hf_nx, hf_ny, hf_bands;   // hf_ny = rows of ONE band
  float hf_inv_cell, hf_x0, hf_y0, hf_cell;
  float hf_lo, hf_hi;              // lowest / highest height of the whole field: the march starts and ends inside this slab
  float trunk_half[3], foot_radius, upper_len, lower_len;
  float hip_origin[4][3], thigh_y[4];
};

// one image's primitives, world frame
struct Prims {
  float p[3], R[9];                // base position, rotation (rows: world = p + R local)
  float o1[4][3], o2[4][3], o3[4][3], pf[4][3];
  float br2;                       // squared radius of the bounding sphere around p
};

// the camera inverse: world ray of a pixel, and the depth-buffer value of a point
struct Camera {
  float eye[3], r0[3], r1[3], r2[3], t2;   // view rotation rows, z translation
  float p0, p5, p8, p9, p10, p11, p14, p15;
};

inline RenderScene make_render_scene(const KCfg& K, const ModelF& M, const float* hf, float lo, float hi) {
  RenderScene S;
  S.hf = hf;
  S.terrain = (K.terrain == 1 && hf) ? 1 : 0;
  S.hf_nx = K.hf_nx; S.hf_ny = K.hf_ny; S.hf_bands = K.hf_bands > 1 ? K.hf_bands : 1;
  S.hf_inv_cell = K.hf_inv_cell; S.hf_x0 = K.hf_x0; S.hf_y0 = K.hf_y0; S.hf_cell = K.hf_cell;
  S.hf_lo = lo; S.hf_hi = hi;
  for (int k = 0; k < 3; k++) S.trunk_half[k] = K.trunk_half[k];
  S.foot_radius = K.foot_radius; S.upper_len = K.upper_len; S.lower_len = K.lower_len;
  for (int l = 0; l < 4; l++) {
    for (int k = 0; k < 3; k++) S.hip_origin[l][k] = M.hip_origin[l][k];
    S.thigh_y[l] = M.thigh_y[l];
  }
  return S;
}

// ---- small vector helpers ------------------------------------------------------------------------------------------------------
ETG_HD float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
ETG_HD void sub3(const float* a, const float* b, float* o) { o[0] = a[0] - b[0]; o[1] = a[1] - b[1]; o[2] = a[2] - b[2]; }
ETG_HD float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
ETG_HD void to_world(const Prims& P, const float* v, float* o) {
  for (int i = 0; i < 3; i++) o[i] = P.p[i] + P.R[3 * i] * v[0] + P.R[3 * i + 1] * v[1] + P.R[3 * i + 2] * v[2];
}

// ---- primitives of one state row -----------------------------------------------------------------------------------------------
ETG_HD void build_prims(const RenderScene& S, const float* st, Prims& P) {
  const float x = st[3], y = st[4], z = st[5], w = st[6];
  for (int k = 0; k < 3; k++) P.p[k] = st[k];
  P.R[0] = 1.0f - 2.0f * (y * y + z * z); P.R[1] = 2.0f * (x * y - z * w); P.R[2] = 2.0f * (x * z + y * w);
  P.R[3] = 2.0f * (x * y + z * w); P.R[4] = 1.0f - 2.0f * (x * x + z * z); P.R[5] = 2.0f * (y * z - x * w);
  P.R[6] = 2.0f * (x * z - y * w); P.R[7] = 2.0f * (y * z + x * w); P.R[8] = 1.0f - 2.0f * (x * x + y * y);
  const float* th = S.trunk_half;
  float br2 = th[0] * th[0] + th[1] * th[1] + th[2] * th[2];
  for (int l = 0; l < 4; l++) {
    float sa, ca, sh, ch, sk, ck;
    sincosf(st[13 + 3 * l], &sa, &ca);
    sincosf(st[14 + 3 * l], &sh, &ch);
    sincosf(st[15 + 3 * l], &sk, &ck);
    const float shk = sh * ck + ch * sk, chk = ch * ck - sh * sk;
    // leg_geometry (etg_core16.h), base frame
    const float* o1 = S.hip_origin[l];
    const float sy = S.thigh_y[l], lu = S.upper_len, ll = S.lower_len;
    const float o2[3] = {o1[0], o1[1] + sy * ca, o1[2] + sy * sa};
    const float o3[3] = {o2[0] - lu * sh, o2[1] + lu * sa * ch, o2[2] - lu * ca * ch};
    const float pf[3] = {o3[0] - ll * shk, o3[1] + ll * sa * chk, o3[2] - ll * ca * chk};
    to_world(P, o1, P.o1[l]);
    to_world(P, o2, P.o2[l]);
    to_world(P, o3, P.o3[l]);
    to_world(P, pf, P.pf[l]);
    // bounding sphere around p (a rotation keeps distances: measure them in the base frame)
    const float e1 = sqrtf(dot3(o1, o1)) + kHipRadius, e2 = sqrtf(dot3(o2, o2)) + kThighRadius;
    const float e3 = sqrtf(dot3(o3, o3)) + kThighRadius, e4 = sqrtf(dot3(pf, pf)) + fmaxf(S.foot_radius, kCalfRadius);
    br2 = fmaxf(fmaxf(br2, e1 * e1), fmaxf(e2 * e2, fmaxf(e3 * e3, e4 * e4)));
  }
  P.br2 = br2 * 1.0001f;
}

// ---- camera --------------------------------------------------------------------------------------------------------------------
// view: gluLookAt-style rigid transform, proj: a perspective projection (clip w = -z_eye), both column-major [16]
ETG_HD void make_camera(const float* V, const float* Pm, Camera& c) {
  for (int k = 0; k < 3; k++) { c.r0[k] = V[4 * k]; c.r1[k] = V[4 * k + 1]; c.r2[k] = V[4 * k + 2]; }
  const float t0 = V[12], t1 = V[13];
  c.t2 = V[14];
  for (int k = 0; k < 3; k++) c.eye[k] = -(t0 * c.r0[k] + t1 * c.r1[k] + c.t2 * c.r2[k]);
  c.p0 = Pm[0]; c.p5 = Pm[5]; c.p8 = Pm[8]; c.p9 = Pm[9]; c.p10 = Pm[10]; c.p11 = Pm[11]; c.p14 = Pm[14]; c.p15 = Pm[15];
}
// unit world direction of the ray through the centre of pixel (px, py); row 0 is the top row
ETG_HD void pixel_ray(const Camera& c, int px, int py, int W, int H, float* d) {
  const float nx = ((float)px + 0.5f) * (2.0f / (float)W) - 1.0f;
  const float ny = 1.0f - ((float)py + 0.5f) * (2.0f / (float)H);
  const float xc = (nx + c.p8) / c.p0, yc = (ny + c.p9) / c.p5;
  for (int k = 0; k < 3; k++) d[k] = xc * c.r0[k] + yc * c.r1[k] - c.r2[k];
  const float inv = 1.0f / sqrtf(dot3(d, d));
  for (int k = 0; k < 3; k++) d[k] *= inv;
}
// OpenGL depth-buffer value 0.5 z_ndc + 0.5 of a world point (pybullet's depth image), clamped to [0, 1]
ETG_HD float depth_value(const Camera& c, const float* q) {
  const float ze = dot3(c.r2, q) + c.t2;
  const float cz = c.p10 * ze + c.p14, cw = c.p11 * ze + c.p15;
  return clamp01(0.5f * cz / cw + 0.5f);
}

// ---- ray / primitive intersections: the nearest root in (tmin, t) replaces t --------------------------------------------------
ETG_HD bool ray_sphere(const float* o, const float* d, const float* c, float r, float tmin, float& t) {
  float oc[3];
  sub3(o, c, oc);
  const float b = dot3(oc, d), cc = dot3(oc, oc) - r * r, h = b * b - cc;
  if (!(h >= 0.0f)) return false;
  const float s = sqrtf(h);
  const float tn = -b - s, tf = -b + s;
  const float th = tn > tmin ? tn : tf;
  if (th > tmin && th < t) { t = th; return true; }
  return false;
}
// capsule a -> b of radius r = cylinder + two end spheres
ETG_HD bool ray_capsule(const float* o, const float* d, const float* a, const float* b, float r, float tmin, float& t) {
  float ba[3], oa[3];
  sub3(b, a, ba);
  sub3(o, a, oa);
  const float baba = dot3(ba, ba), bard = dot3(ba, d), baoa = dot3(ba, oa), rdoa = dot3(d, oa), oaoa = dot3(oa, oa);
  const float A = baba - bard * bard;
  bool hit = false;
  if (A > 1e-9f * baba) {
    const float B = baba * rdoa - baoa * bard, C = baba * oaoa - baoa * baoa - r * r * baba;
    const float h = B * B - A * C;
    if (h >= 0.0f) {
      const float s = sqrtf(h);
      const float tn = (-B - s) / A, tf = (-B + s) / A;
      const float yn = baoa + tn * bard, yf = baoa + tf * bard;
      if (tn > tmin && tn < t && yn > 0.0f && yn < baba) { t = tn; hit = true; }
      else if (tf > tmin && tf < t && yf > 0.0f && yf < baba) { t = tf; hit = true; }
    }
  }
  hit |= ray_sphere(o, d, a, r, tmin, t);
  hit |= ray_sphere(o, d, b, r, tmin, t);
  return hit;
}
// the trunk box (half extents th, centred on the base frame); n: the outward normal of the face hit, world frame
ETG_HD bool ray_box(const Prims& P, const float* th, const float* o, const float* d, float tmin, float& t, float* n) {
  float rel[3], ol[3], dl[3];
  sub3(o, P.p, rel);
  for (int k = 0; k < 3; k++) {
    ol[k] = P.R[k] * rel[0] + P.R[3 + k] * rel[1] + P.R[6 + k] * rel[2];
    dl[k] = P.R[k] * d[0] + P.R[3 + k] * d[1] + P.R[6 + k] * d[2];
  }
  float tn = -kFar, tf = kFar;
  int an = 0, af = 0;
  float sn = 1.0f, sf = 1.0f;
  for (int k = 0; k < 3; k++) {
    if (fabsf(dl[k]) < 1e-12f) {
      if (fabsf(ol[k]) > th[k]) return false;
      continue;
    }
    const float inv = 1.0f / dl[k];
    float t1 = (-th[k] - ol[k]) * inv, t2 = (th[k] - ol[k]) * inv;
    float s1 = -1.0f;                        // the face the ray enters through at t1
    if (t1 > t2) { const float tmp = t1; t1 = t2; t2 = tmp; s1 = 1.0f; }
    if (t1 > tn) { tn = t1; an = k; sn = s1; }
    if (t2 < tf) { tf = t2; af = k; sf = -s1; }
  }
  if (!(tn <= tf)) return false;
  const bool front = tn > tmin;
  const float th_ = front ? tn : tf;
  const int ax = front ? an : af;
  const float s = front ? sn : sf;
  if (!(th_ > tmin && th_ < t)) return false;
  t = th_;
  n[0] = s * (ax == 0 ? P.R[0] : ax == 1 ? P.R[1] : P.R[2]);
  n[1] = s * (ax == 0 ? P.R[3] : ax == 1 ? P.R[4] : P.R[5]);
  n[2] = s * (ax == 0 ? P.R[6] : ax == 1 ? P.R[7] : P.R[8]);
  return true;
}

// nearest robot primitive along the ray in (tmin, t): its segment id (or SEG_SKY) and, when n is given, its world normal
ETG_HD int hit_robot(const RenderScene& S, const Prims& P, const float* o, const float* d, float tmin, float& t, float* n) {
  {  // bounding sphere: most ground and sky rays stop here
    float oc[3];
    sub3(o, P.p, oc);
    const float b = dot3(oc, d), c = dot3(oc, oc) - P.br2;
    if (c > 0.0f && (b > 0.0f || b * b - c < 0.0f)) return SEG_SKY;
  }
  int seg = SEG_SKY, leg = 0, part = 0;
  float nb[3];
  if (ray_box(P, S.trunk_half, o, d, tmin, t, nb)) seg = SEG_TRUNK;
  for (int l = 0; l < 4; l++) {
    if (ray_sphere(o, d, P.o1[l], kHipRadius, tmin, t)) { seg = SEG_LEG0; leg = l; part = PART_HIP; }
    if (ray_capsule(o, d, P.o2[l], P.o3[l], kThighRadius, tmin, t)) { seg = SEG_LEG0; leg = l; part = PART_THIGH; }
    if (ray_capsule(o, d, P.o3[l], P.pf[l], kCalfRadius, tmin, t)) { seg = SEG_LEG0; leg = l; part = PART_CALF; }
    if (ray_sphere(o, d, P.pf[l], S.foot_radius, tmin, t)) { seg = SEG_LEG0; leg = l; part = PART_FOOT; }
  }
  if (seg != SEG_LEG0) {
    if (seg == SEG_TRUNK && n) { n[0] = nb[0]; n[1] = nb[1]; n[2] = nb[2]; }
    return seg;
  }
  if (n) {  // normal of the leg primitive hit: from the nearest point of its axis segment (a sphere: a zero-length segment)
    float q[3];
    for (int k = 0; k < 3; k++) q[k] = o[k] + t * d[k];
    const float* a = part == PART_HIP ? P.o1[leg] : part == PART_THIGH ? P.o2[leg] : part == PART_CALF ? P.o3[leg] : P.pf[leg];
    const float* b = part == PART_THIGH ? P.o3[leg] : part == PART_CALF ? P.pf[leg] : a;
    float ba[3], qa[3];
    sub3(b, a, ba);
    sub3(q, a, qa);
    const float bb = dot3(ba, ba);
    const float u = bb > 0.0f ? clamp01(dot3(qa, ba) / bb) : 0.0f;
    for (int k = 0; k < 3; k++) n[k] = qa[k] - u * ba[k];
    const float nn = dot3(n, n);
    const float inv = nn > 0.0f ? 1.0f / sqrtf(nn) : 0.0f;
    for (int k = 0; k < 3; k++) n[k] *= inv;
  }
  return SEG_LEG0 + 4 * leg + part;
}

// ---- terrain -------------------------------------------------------------------------------------------------------------------
// bilinear height of band `band` at (x, y), clamped at the border exactly as heightfield_fetch (etg_layout.h); grad: its gradient
ETG_HD float hf_height(const RenderScene& S, int band, float x, float y, float* grad) {
  const float* hf = S.hf + (size_t)band * S.hf_ny * S.hf_nx;
  float fx = (x - S.hf_x0) * S.hf_inv_cell, fy = (y - S.hf_y0) * S.hf_inv_cell;
  fx = fminf(fmaxf(fx, 0.0f), (float)(S.hf_nx - 1));
  fy = fminf(fmaxf(fy, 0.0f), (float)(S.hf_ny - 1));
  int ix = (int)fx, iy = (int)fy;
  if (ix > S.hf_nx - 2) ix = S.hf_nx - 2;
  if (iy > S.hf_ny - 2) iy = S.hf_ny - 2;
  const float tx = fx - (float)ix, ty = fy - (float)iy;
  const float h00 = hf[iy * S.hf_nx + ix], h10 = hf[iy * S.hf_nx + ix + 1];
  const float h01 = hf[(iy + 1) * S.hf_nx + ix], h11 = hf[(iy + 1) * S.hf_nx + ix + 1];
  if (grad) {
    grad[0] = ((1 - ty) * (h10 - h00) + ty * (h11 - h01)) * S.hf_inv_cell;
    grad[1] = ((1 - tx) * (h01 - h00) + tx * (h11 - h10)) * S.hf_inv_cell;
  }
  return (1 - tx) * (1 - ty) * h00 + tx * (1 - ty) * h10 + (1 - tx) * ty * h01 + tx * ty * h11;
}
ETG_HD float above_terrain(const RenderScene& S, int band, const float* o, const float* d, float t) {
  return o[2] + t * d[2] - hf_height(S, band, o[0] + t * d[0], o[1] + t * d[1], nullptr);
}

// nearest terrain point along the ray within tmax: the plane z = 0, or the band marched at most one cell per step between
// the heights' slab [hf_lo, hf_hi] and tmax, the crossing refined by bisection.  n: the terrain normal there.
ETG_HD bool hit_terrain(const RenderScene& S, int band, const float* o, const float* d, float tmax, float& t, float* n) {
  if (!S.terrain) {
    if (!(d[2] < -1e-12f)) return false;
    const float tp = -o[2] / d[2];
    if (!(tp > 0.0f && tp < tmax)) return false;
    t = tp;
    n[0] = 0.0f; n[1] = 0.0f; n[2] = 1.0f;
    return true;
  }
  float t0 = 0.0f, t1 = tmax;
  if (d[2] < -1e-12f) {
    t0 = fmaxf(t0, (S.hf_hi + kSlabMargin - o[2]) / d[2]);
    t1 = fminf(t1, (S.hf_lo - kSlabMargin - o[2]) / d[2]);
  } else if (o[2] > S.hf_hi + kSlabMargin) {
    return false;
  }
  if (!(t1 > t0)) return false;
  int steps = (int)ceilf((t1 - t0) / S.hf_cell);
  steps = steps < 1 ? 1 : steps > kMaxMarch ? kMaxMarch : steps;
  const float dt = (t1 - t0) / (float)steps;
  float ta = t0, tb = t0;
  if (above_terrain(S, band, o, d, ta) < 0.0f) return false;   // the camera is inside the terrain
  bool found = false;
  for (int i = 1; i <= steps; i++) {
    tb = t0 + (float)i * dt;
    if (above_terrain(S, band, o, d, tb) <= 0.0f) { found = true; break; }
    ta = tb;
  }
  if (!found) return false;
  for (int i = 0; i < kBisect; i++) {   // above at ta, not above at tb
    const float tm = 0.5f * (ta + tb);
    if (above_terrain(S, band, o, d, tm) <= 0.0f) tb = tm;
    else ta = tm;
  }
  t = tb;
  float g[2];
  hf_height(S, band, o[0] + t * d[0], o[1] + t * d[1], g);
  const float inv = 1.0f / sqrtf(g[0] * g[0] + g[1] * g[1] + 1.0f);
  n[0] = -g[0] * inv; n[1] = -g[1] * inv; n[2] = inv;
  return true;
}

// ---- shading -------------------------------------------------------------------------------------------------------------------
ETG_HD void albedo(int seg, const float* q, float* c) {
  if (seg == SEG_TERRAIN) {
    const int cx = (int)floorf(q[0] * (1.0f / kChecker)), cy = (int)floorf(q[1] * (1.0f / kChecker));
    const float g = ((cx + cy) & 1) ? kGroundB : kGroundA;
    c[0] = g; c[1] = g; c[2] = g;
  } else if (seg == SEG_TRUNK) {
    c[0] = kTrunkR; c[1] = kTrunkG; c[2] = kTrunkB;
  } else {
    const int part = (seg - SEG_LEG0) & 3;
    c[0] = part == PART_HIP ? kHipR : part == PART_THIGH ? kThighR : part == PART_CALF ? kCalfR : kFootR;
    c[1] = part == PART_HIP ? kHipG : part == PART_THIGH ? kThighG : part == PART_CALF ? kCalfG : kFootG;
    c[2] = part == PART_HIP ? kHipB : part == PART_THIGH ? kThighB : part == PART_CALF ? kCalfB : kFootB;
  }
}
ETG_HD uint32_t pack_rgba(float r, float g, float b) {
  const uint32_t R = (uint32_t)(clamp01(r) * 255.0f + 0.5f), G = (uint32_t)(clamp01(g) * 255.0f + 0.5f),
                 B = (uint32_t)(clamp01(b) * 255.0f + 0.5f);
  return R | (G << 8) | (B << 16) | (255u << 24);
}

// one pixel: rgba (bytes r, g, b, a in memory order), the depth-buffer value and the segment id
ETG_HD void shade_pixel(const RenderScene& S, const Prims& P, const Camera& cam, int band, int px, int py, int W, int H,
                        uint32_t& rgba, float& depth, int& seg) {
  float d[3], n[3] = {0.0f, 0.0f, 1.0f}, nt[3];
  pixel_ray(cam, px, py, W, H, d);
  float t = kDrawDist;
  seg = hit_robot(S, P, cam.eye, d, 0.0f, t, n);
  if (hit_terrain(S, band, cam.eye, d, t, t, nt)) {
    seg = SEG_TERRAIN;
    n[0] = nt[0]; n[1] = nt[1]; n[2] = nt[2];
  }
  if (seg == SEG_SKY) {
    rgba = pack_rgba(kSkyR, kSkyG, kSkyB);
    depth = 1.0f;
    return;
  }
  float q[3];
  for (int k = 0; k < 3; k++) q[k] = cam.eye[k] + t * d[k];
  depth = depth_value(cam, q);
  const float L[3] = {kLightX, kLightY, kLightZ};
  float diff = fmaxf(dot3(n, L), 0.0f);
  if (diff > 0.0f) {   // one shadow ray toward the light, against the robot only
    float s[3];
    for (int k = 0; k < 3; k++) s[k] = q[k] + kShadowLift * n[k];
    float ts = kFar;
    if (hit_robot(S, P, s, L, 0.0f, ts, nullptr) != SEG_SKY) diff = 0.0f;
  }
  float c[3];
  albedo(seg, q, c);
  const float k = kAmbient + kDiffuse * diff;
  rgba = pack_rgba(c[0] * k, c[1] * k, c[2] * k);
}

// terrain band of an env id (robot e walks on band e % hf_bands)
ETG_HD int band_of(const RenderScene& S, int env_id) {
  const int b = env_id % S.hf_bands;
  return b < 0 ? b + S.hf_bands : b;
}

// lowest / highest height of a heightfield (host)
inline void height_range(const float* h, size_t count, float& lo, float& hi) {
  lo = count ? h[0] : 0.0f;
  hi = lo;
  for (size_t i = 1; i < count; i++) { lo = fminf(lo, h[i]); hi = fmaxf(hi, h[i]); }
}

}  // namespace render
}  // namespace etg

// the kernel's launcher (etg_render.hip); arguments as etg_render (include/etgsim_render.h), already checked by the caller
#if defined(__HIPCC__)
hipError_t etg_render_launch(const etg::render::RenderScene& S, const float* state, const int* env_ids, int n, const float* view,
                             const float* proj, int width, int height, uint8_t* rgba, float* depth, int* seg, hipStream_t stream);
#endif
