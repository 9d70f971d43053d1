// lcr_render.hip -- image observations: a small ray-caster for the two observation cameras of every env (240x320 unless lcr_config.image_width / image_height say otherwise)
// (get_observation, envs/reach_cube_env.py:288-292: renderer.update_scene(camera="camera_front"/"camera_top"); render())
// and for the 640x640 `camera_vizu` frame of render() (envs/reach_cube_env.py:350-355).
//
// It is an APPROXIMATE restatement, not MuJoCo's OpenGL renderer (which cannot run here): pinhole cameras with the
// poses of the scene xmls (reach_cube.xml:29-31) and MuJoCo's default fovy 45 deg; checker floor (texrepeat 5 -> 0.1 m
// squares, reach_cube.xml:14-16), gradient sky, the cube(s) as exact oriented boxes, the arm -- round 5 -- as the bounding boxes of its seven collision
// hulls (base_link, link_1 .. link_6: mesh extents of the golden model file, follower.xml:54-97; the 20 STL meshes themselves are not shipped; rounds 1-4
// drew capsules between the link origins), ambient 0.3 + headlight 0.6 Lambert shading, no shadows.
//
// Mapping: a workgroup owns one env's 2 H image rows (both frames; small frames: up to four envs); a wave handles one BAND of 4 rows at a time and writes its 12 W
// bytes (3 840 at 320 wide) with non-temporal 16-B stores.  What does not depend on the env -- floor, sky and the arm's base -- is rendered once into a
// cached frame pair, and bands no other primitive touches are plain copies of it.  The per-env scene (FK of the arm, cube frames, per camera the
// ray-test constants and the screen-space silhouette of every primitive) is built once per workgroup in LDS; culling is wave-uniform (per band and
// 16-pixel column), only 16 x 4 tiles that a silhouette touches are ray-cast.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "lcr_arm.h"
#include "lcr_device.h"
#include "lcr_wrist_pose.h"

using namespace lcrdev;

// This file is compiled as five units (build.py): LCR_RENDER_PART 0 = the 320 x 240 frame kernel and the small kernels, 1 = the frame kernels for run-time sizes, 3 = the
// kernels that draw the depth / segmentation planes (include/lcr.h: lcr_enable_image_planes), 4 = the kernels that draw with a look (lcr_enable_look), 5 = the kernels of the
// wrist camera (lcr_enable_wrist_camera); undefined = everything in one unit (the tools that compile this file on its own)
#ifndef LCR_RENDER_PART
#define LCR_RENDER_PART 2
#endif
#define LCR_RENDER_SMALL (LCR_RENDER_PART == 0 || LCR_RENDER_PART == 2)
#define LCR_RENDER_SIZED (LCR_RENDER_PART == 1 || LCR_RENDER_PART == 2)
#define LCR_RENDER_PLANES (LCR_RENDER_PART == 3 || LCR_RENDER_PART == 2)
#define LCR_RENDER_LOOK (LCR_RENDER_PART == 4 || LCR_RENDER_PART == 2)
#define LCR_RENDER_WRIST (LCR_RENDER_PART == 5 || LCR_RENDER_PART == 2)

namespace {

constexpr int NARM = 7;    // base_link, link_1 .. link_6 as the bounding boxes of their collision hulls (lcr_model_gen.h ARMB*: model_golden.json "mesh_aabb")
constexpr int NBOX = NARM + 3;      // the arm boxes, then cube, second cube (Stack), target marker (Push / PickPlace)
constexpr int NPRIM = NBOX;
constexpr int BASE = 0;    // the base box is the same in every env: part of the cached background, ray-cast only where another primitive may hide it / hide behind it

struct Scene {
    f3 bc[NBOX], bX[NBOX], bY[NBOX], bZ[NBOX], bh[NBOX];
    f3 bcol[NBOX];
    float balpha[NBOX];
    int nbox;
    int marker;   // index of the translucent target marker among the boxes, -1 if the task has none
    // per camera: the ray direction in the box frame is affine in the pixel, dl = C0 + sy B + sx A:  A(3) ol.x | B(3) ol.y | C0(3) ol.z | half(3) alpha
    // (ol = box-frame coordinates of the camera position)
    __attribute__((aligned(16))) float boxc[2][NBOX][16];
    // culling record per camera and primitive, read back by the primitive's lane for every band:
    // y0 y1 x0 x1 of the screen bounding box | stadium au av du R | du/dv 1/dv strip half-width, flat flag
    __attribute__((aligned(16))) float cull[2][NPRIM][12];
};

DEV void arm_box(int i, f3 &c, f3 &h) {
    const float bc[NARM][3] = {{lcrm::ARMB0cx, lcrm::ARMB0cy, lcrm::ARMB0cz}, {lcrm::ARMB1cx, lcrm::ARMB1cy, lcrm::ARMB1cz}, {lcrm::ARMB2cx, lcrm::ARMB2cy, lcrm::ARMB2cz},
                               {lcrm::ARMB3cx, lcrm::ARMB3cy, lcrm::ARMB3cz}, {lcrm::ARMB4cx, lcrm::ARMB4cy, lcrm::ARMB4cz}, {lcrm::ARMB5cx, lcrm::ARMB5cy, lcrm::ARMB5cz},
                               {lcrm::ARMB6cx, lcrm::ARMB6cy, lcrm::ARMB6cz}};
    const float bh[NARM][3] = {{lcrm::ARMB0hx, lcrm::ARMB0hy, lcrm::ARMB0hz}, {lcrm::ARMB1hx, lcrm::ARMB1hy, lcrm::ARMB1hz}, {lcrm::ARMB2hx, lcrm::ARMB2hy, lcrm::ARMB2hz},
                               {lcrm::ARMB3hx, lcrm::ARMB3hy, lcrm::ARMB3hz}, {lcrm::ARMB4hx, lcrm::ARMB4hy, lcrm::ARMB4hz}, {lcrm::ARMB5hx, lcrm::ARMB5hy, lcrm::ARMB5hz},
                               {lcrm::ARMB6hx, lcrm::ARMB6hy, lcrm::ARMB6hz}};
    c = mk(bc[i][0], bc[i][1], bc[i][2]); h = mk(bh[i][0], bh[i][1], bh[i][2]);
}

// the base box (body frame of base_link: Rz(-90 deg) at the origin, follower.xml:51)
DEV void base_box(f3 &c, f3 &X, f3 &Y, f3 &Z, f3 &h) {
    X = mk(0.f, -1.f, 0.f); Y = mk(1.f, 0.f, 0.f); Z = mk(0.f, 0.f, 1.f);
    f3 lc;
    arm_box(0, lc, h);
    c = axpy(lc.x, X, axpy(lc.y, Y, lc.z * Z));
}

DEV void build_scene(const LcrDev &P, int env, Scene &S) {
    const int N = P.n;
    float q[6];
    for (int j = 0; j < 6; j++) q[j] = P.qpos[(size_t)j * N + env];
    ArmFrames F;
    arm_frames(q, F);
    base_box(S.bc[0], S.bX[0], S.bY[0], S.bZ[0], S.bh[0]);
    S.bcol[0] = mk(0.8f, 0.8f, 0.8f); S.balpha[0] = 1.f;
    for (int i = 1; i < NARM; i++) {   // link_i: frame i - 1 of the chain
        f3 lc;
        arm_box(i, lc, S.bh[i]);
        S.bc[i] = local_point(F, i - 1, lc.x, lc.y, lc.z);
        S.bX[i] = F.X[i - 1]; S.bY[i] = F.Y[i - 1]; S.bZ[i] = F.Z[i - 1];
        const float g = i >= 5 ? 0.75f : 0.8f;   // the two fingers a shade darker
        S.bcol[i] = mk(g, g, g);
        S.balpha[i] = 1.f;
    }
    const int ncube = P.task == 4 ? 2 : 1;
    int nb = NARM;
    for (int c = 0; c < ncube; c++) {
        const float *qp = P.qpos + (size_t)(6 + 7 * c) * N + env;
        float cq[4] = {qp[3 * (size_t)N], qp[4 * (size_t)N], qp[5 * (size_t)N], qp[6 * (size_t)N]};
        CubeRot R = quat_to_cols(cq);
        S.bc[nb] = mk(qp[0], qp[N], qp[2 * (size_t)N]);
        S.bX[nb] = R.X; S.bY[nb] = R.Y; S.bZ[nb] = R.Z;
        S.bh[nb] = mk(0.015f, 0.015f, 0.015f);
        S.bcol[nb] = c == 0 ? mk(0.5f, 0.f, 0.f) : mk(0.f, 0.f, 0.5f);  // reach_cube.xml:26 rgba / stack_two_cubes.xml:34
        S.balpha[nb] = 1.f;
        nb++;
    }
    S.marker = P.has_target ? nb : -1;
    if (P.has_target) {  // push_cube.xml:35 cylinder r=0.035 h=0.01 / pick_place_cube.xml:35 box 0.015^3, rgba 0 0 1 0.3
        S.bc[nb] = mk(P.target[env], P.target[N + env], P.target[2 * (size_t)N + env]);
        S.bX[nb] = mk(1.f, 0.f, 0.f); S.bY[nb] = mk(0.f, 1.f, 0.f); S.bZ[nb] = mk(0.f, 0.f, 1.f);
        S.bh[nb] = P.task == 2 ? mk(0.035f, 0.035f, 0.01f) : mk(0.015f, 0.015f, 0.015f);
        S.bcol[nb] = mk(0.f, 0.f, 1.f);
        S.balpha[nb] = 0.3f;
        nb++;
    }
    S.nbox = nb;
}

// ray-test constants of one box for one camera (16 floats, see Scene::boxc)
DEV void box_consts(const LcrCam &C, f3 bc, f3 bX, f3 bY, f3 bZ, f3 bh, float alpha, float *c) {
    const f3 ro = mk(C.px, C.py, C.pz), CX = mk(C.xx, C.xy, C.xz), CY = mk(C.yx, C.yy, C.yz), CZ = mk(C.zx, C.zy, C.zz);
    const f3 d = ro - bc;
    c[0] = dot(bX, CX); c[1] = dot(bY, CX); c[2] = dot(bZ, CX); c[3] = dot(bX, d);
    c[4] = dot(bX, CY); c[5] = dot(bY, CY); c[6] = dot(bZ, CY); c[7] = dot(bY, d);
    c[8] = -dot(bX, CZ); c[9] = -dot(bY, CZ); c[10] = -dot(bZ, CZ); c[11] = dot(bZ, d);
    c[12] = bh.x; c[13] = bh.y; c[14] = bh.z; c[15] = alpha;
}

// per-camera constants of ONE primitive (called by one thread per (camera, primitive)): ray-test constants, screen bounding box, and for the arm boxes the
// 2D stadium that bounds the 8 projected corners -- axis through the projected centres of the two faces across the box's longest edge, half-width = the
// largest distance of a corner from that axis, ends at the extreme corners along it
DEV void build_prim(const LcrCam &C, int cam, int W, int H, Scene &S, int k) {
    float *cl = S.cull[cam][k];
    for (int i = 4; i < 12; i++) cl[i] = 0.f;
    if (k >= S.nbox) { cl[0] = (float)H; cl[1] = -1.f; cl[2] = (float)W; cl[3] = -1.f; return; }
    box_consts(C, S.bc[k], S.bX[k], S.bY[k], S.bZ[k], S.bh[k], S.balpha[k], S.boxc[cam][k]);
    const f3 ro = mk(C.px, C.py, C.pz), CX = mk(C.xx, C.xy, C.xz), CY = mk(C.yx, C.yy, C.yz), CZ = mk(C.zx, C.zy, C.zz);
    float uv[8][2];
    bool ok = true;
    float x0 = 1e30f, x1 = -1e30f, y0 = 1e30f, y1 = -1e30f;
    for (int i = 0; i < 8; i++) {
        const f3 p = axpy((i & 1) ? S.bh[k].x : -S.bh[k].x, S.bX[k], axpy((i & 2) ? S.bh[k].y : -S.bh[k].y, S.bY[k],
                     axpy((i & 4) ? S.bh[k].z : -S.bh[k].z, S.bZ[k], S.bc[k])));
        const f3 e = p - ro;
        const float xc = dot(e, CX), yc = dot(e, CY);
        float zc = -dot(e, CZ);
        if (zc < 0.02f) { ok = false; zc = 0.02f; }
        const float inv = 1.0f / (zc * C.s);
        uv[i][0] = 0.5f * W + xc * inv - 0.5f; uv[i][1] = 0.5f * H - yc * inv - 0.5f;   // pixel (px, row) has its centre at (px, row)
        x0 = fminf(x0, uv[i][0]); x1 = fmaxf(x1, uv[i][0]); y0 = fminf(y0, uv[i][1]); y1 = fmaxf(y1, uv[i][1]);
    }
    if (!ok) { cl[0] = 0.f; cl[1] = (float)(H - 1); cl[2] = 0.f; cl[3] = (float)(W - 1); cl[7] = 1e15f; cl[10] = 1e15f; cl[11] = 1.f; return; }
    cl[0] = floorf(y0 - 1.f); cl[1] = ceilf(y1 + 1.f); cl[2] = floorf(x0 - 1.f); cl[3] = ceilf(x1 + 1.f);
    if (k >= NARM) return;   // cubes, marker: the bounding box is all there is
    const int ax = S.bh[k].x >= S.bh[k].y ? (S.bh[k].x >= S.bh[k].z ? 0 : 2) : (S.bh[k].y >= S.bh[k].z ? 1 : 2);
    const int bit = 1 << ax;
    float a0u = 0.f, a0v = 0.f, a1u = 0.f, a1v = 0.f;
    for (int i = 0; i < 8; i++) {
        if (i & bit) { a1u += 0.25f * uv[i][0]; a1v += 0.25f * uv[i][1]; }
        else { a0u += 0.25f * uv[i][0]; a0v += 0.25f * uv[i][1]; }
    }
    float au = a1u - a0u, av = a1v - a0v;
    const float len = sqrtf(au * au + av * av);
    if (len > 1e-3f) { au /= len; av /= len; } else { au = 1.f; av = 0.f; }
    float smin = 1e30f, smax = -1e30f, wmax = 0.f;
    for (int i = 0; i < 8; i++) {
        const float eu = uv[i][0] - a0u, ev = uv[i][1] - a0v;
        const float sc = eu * au + ev * av;
        smin = fminf(smin, sc); smax = fmaxf(smax, sc);
        wmax = fmaxf(wmax, fabsf(eu * av - ev * au));
    }
    const float du = (smax - smin) * au, dv = (smax - smin) * av, R = wmax + 1.0f;
    const bool flat = fabsf(dv) < 1e-4f;
    const float inv_dv = flat ? 0.f : 1.0f / dv;
    cl[4] = a0u + smin * au; cl[5] = a0v + smin * av; cl[6] = du; cl[7] = R;
    // the stadium lies inside the infinite strip of half-width R around its axis: on row y the strip spans cx(y) -+ R / |sin(axis, row)|
    cl[8] = du * inv_dv; cl[9] = inv_dv; cl[10] = flat ? 1e15f : R * sqrtf(du * du + dv * dv) * fabsf(inv_dv); cl[11] = flat ? 1.f : 0.f;
}

// rgb in [0,1] -> 0x00BBGGRR with v_cvt_pk_u8_f32 (saturating float->byte conversion and byte insert in one instruction)
DEV unsigned pack_rgb(f3 c) {
    unsigned v = 0u;
    v = __builtin_amdgcn_cvt_pk_u8_f32(c.x * 255.f, 0, v);
    v = __builtin_amdgcn_cvt_pk_u8_f32(c.y * 255.f, 1, v);
    v = __builtin_amdgcn_cvt_pk_u8_f32(c.z * 255.f, 2, v);
    return v;
}

// slab test of one box along the UN-normalised ray ro + t d, d = C0 + sy B + sx A in the box frame (c = Scene::boxc record).  Returns the entry parameter
// (>= 0 means hit when it is also <= the exit) and |n . d| of the entry face: the face's normal is a box axis, so the headlight's Lambert term is a component of
// the box-frame direction -- no normal vector is ever formed.
DEV bool box_hit(const float *c, float sx, float sy, float tlimit, float &tmin, float &ld) {
    const float dx = fmaf(sx, c[0], fmaf(sy, c[4], c[8])), dy = fmaf(sx, c[1], fmaf(sy, c[5], c[9])), dz = fmaf(sx, c[2], fmaf(sy, c[6], c[10]));
    const float ix = rcp(fabsf(dx) > 1e-9f ? dx : 1e-9f), iy = rcp(fabsf(dy) > 1e-9f ? dy : 1e-9f), iz = rcp(fabsf(dz) > 1e-9f ? dz : 1e-9f);
    // slab: centre crossing -ol/dl, half width half/|dl|
    const float cx = -c[3] * ix, cy = -c[7] * iy, cz = -c[11] * iz;
    const float hx = c[12] * fabsf(ix), hy = c[13] * fabsf(iy), hz = c[14] * fabsf(iz);
    const float tnx = cx - hx, tny = cy - hy, tnz = cz - hz;
    tmin = fmaxf(tnx, fmaxf(tny, tnz));
    const float tmax = fminf(cx + hx, fminf(cy + hy, cz + hz));
    ld = tmin == tnx ? fabsf(dx) : (tmin == tny ? fabsf(dy) : fabsf(dz));
    return tmin <= tmax && tmin > 0.f && tmin < tlimit;
}

// what a look variant changes in the shading (include/lcr.h: lcr_look_variant); the values every build without a look draws with
struct Shade {
    f3 floor_odd, floor_even, sky, sky_slope;
    float amb, dif;   // ambient + headlight (reach_cube.xml:8)
};
[[maybe_unused]] DEV Shade default_shade() {
    Shade h;
    h.floor_odd = mk(0.2f, 0.3f, 0.4f); h.floor_even = mk(0.1f, 0.2f, 0.3f);
    h.sky = mk(0.15f, 0.25f, 0.35f); h.sky_slope = mk(0.15f, 0.25f, 0.35f);
    h.amb = 0.3f; h.dif = 0.6f;
    return h;
}
// ... and the values of a look variant (lcr_enable_look)
[[maybe_unused]] DEV Shade look_shade(const LcrLookVar &V) {
    Shade h;
    h.floor_odd = mk(V.floor_rgb[0][0], V.floor_rgb[0][1], V.floor_rgb[0][2]); h.floor_even = mk(V.floor_rgb[1][0], V.floor_rgb[1][1], V.floor_rgb[1][2]);
    h.sky = mk(V.sky_rgb[0], V.sky_rgb[1], V.sky_rgb[2]); h.sky_slope = mk(V.sky_slope[0], V.sky_slope[1], V.sky_slope[2]);
    h.amb = V.ambient; h.dif = V.diffuse;
    return h;
}

#if LCR_RENDER_SMALL || LCR_RENDER_LOOK   // (the per-pixel shading of the background and single-frame kernels)
DEV f3 floor_or_sky(f3 ro, f3 d, float inv_len, float &tfloor, const Shade &h) {
    // checker floor below the horizon (builtin checker, 0.1 m squares; its normal is +z so the Lambert term is -d_z / |d|), gradient sky above (unshaded)
    const float rdz = d.z * inv_len;
    if (rdz < -1e-6f) {
        tfloor = -ro.z * rcp(d.z);
        const float fx = fmaf(tfloor, d.x, ro.x), fy = fmaf(tfloor, d.y, ro.y);
        const int cell = ((int)floorf(fx * 10.f) + (int)floorf(fy * 10.f)) & 1;
        const float lam = fminf(fmaf(-h.dif, rdz, h.amb), 1.f);
        return lam * (cell ? h.floor_odd : h.floor_even);
    }
    tfloor = 1e30f;
    const float a = clampf(rdz * 2.f, 0.f, 1.f);
    return mk(h.sky.x + a * h.sky_slope.x, h.sky.y + a * h.sky_slope.y, h.sky.z + a * h.sky_slope.z);
}

// one pixel, every primitive of the scene (cached background: the base only; render(): all): linear rgb in [0,1]
DEV f3 shade_pixel(const LcrCam &C, const float (*boxc)[16], const f3 *bcol, int nbox, int marker, float sx, float sy, const Shade &h) {
    const f3 ro = mk(C.px, C.py, C.pz);
    const f3 d = mk(C.xx * sx + C.yx * sy - C.zx, C.xy * sx + C.yy * sy - C.zy, C.xz * sx + C.yz * sy - C.zz);
    const float inv_len = rsq(dot(d, d));
    float tbest;
    f3 out = floor_or_sky(ro, d, inv_len, tbest, h);
    float talpha = 0.f, tlamd = 0.f;
    for (int k = 0; k < nbox; k++) {
        float tmin, ld;
        if (!box_hit(boxc[k], sx, sy, tbest, tmin, ld)) continue;
        if (k == marker) { tlamd = ld; talpha = boxc[k][15]; }
        else { tbest = tmin; out = fminf(fmaf(h.dif * inv_len, ld, h.amb), 1.f) * bcol[k]; }
    }
    if (talpha > 0.f) out = axpy(talpha * fmaf(h.dif * inv_len, tlamd, h.amb), bcol[marker], (1.f - talpha) * out);
    return out;
}

#endif

// One tile of an observation band: ray-cast the boxes of mask `m` (wave-uniform).  The staged rows already hold the background (floor, sky, base), so a
// lane only reports a colour when its ray hits something else.  `stpx` = this pixel's 3 staged background bytes (read for the translucent target marker
// only).  Returns true and sets rgb when the pixel has to be rewritten.  PLANES: the nearest opaque surface among the floor and the boxes of `m` is reported as well --
// tnear its ray parameter (1e30: sky), knear its box (-1: floor or sky), mhit whether the translucent marker lies in front of it -- whatever the return value.
template <bool PLANES>
DEV bool shade_span(const Scene &S, int cam, int marker, f3 ro, float sx, float sy, f3 d, unsigned m, const unsigned char *stpx, unsigned &rgb, float &tnear, int &knear,
                    bool &mhit, float amb, float dif) {
    float tbest = d.z < -1e-6f ? -ro.z * rcp(d.z) : 1e30f;   // the floor hides what lies below it
    int kbest = -1;
    float lamd = 0.f;   // |n . d| of the nearest hit
    float talpha = 0.f, tlamd = 0.f;
    for (unsigned mm = m; mm; mm &= mm - 1u) {
        const int k = __builtin_ctz(mm);
        float tmin, ld;
        if (box_hit(S.boxc[cam][k], sx, sy, tbest, tmin, ld)) {
            if (k == marker) { tlamd = ld; talpha = S.boxc[cam][k][15]; }     // (the marker is the last box: every opaque primitive has been seen)
            else { tbest = tmin; lamd = ld; kbest = k; }
        }
    }
    if (PLANES) { tnear = tbest; knear = kbest; mhit = talpha > 0.f; }
    const bool draw = kbest > BASE || talpha > 0.f;   // (a pixel whose nearest hit is the base keeps its background bytes)
    if (!__any(draw)) return false;
    const float inv_len = rsq(dot(d, d));
    const float lam = fminf(fmaf(dif * inv_len, lamd, amb), 1.f);  // ambient + headlight (reach_cube.xml:8)
    f3 out = lam * S.bcol[kbest < 0 ? 0 : kbest];
    if (__any(talpha > 0.f)) {   // the translucent marker: over the opaque hit, or over the staged background
        if (kbest <= BASE) out = mk(stpx[0] * (1.f / 255.f), stpx[1] * (1.f / 255.f), stpx[2] * (1.f / 255.f));
        const float tl = fmaf(dif * inv_len, tlamd, amb);
        if (talpha > 0.f) out = axpy(talpha * tl, S.bcol[marker < 0 ? 0 : marker], (1.f - talpha) * out);
    }
    rgb = pack_rgb(out);
    return draw;
}

#if LCR_RENDER_SMALL
// background frames of the two observation cameras -- checker floor, sky and the arm's base: identical for every env and every step, so they
// are rendered ONCE at lcr_create into P.img_bg ([2][H][W][3]; 460 800 B at 320 x 240, L2-resident) and copied band-wise afterwards.
__global__ __launch_bounds__(256) void lcr_render_bg_kernel(LcrDev P, LcrCam front, LcrCam top) {
    const int W = P.img_w, H = P.img_h;
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= 2 * W * H) return;
    const bool is_top = pix >= W * H;
    const int p = is_top ? pix - W * H : pix;
    const int row = p / W, px = p - row * W;
    const LcrCam &C = is_top ? top : front;
    const float sy = -(row + 0.5f - 0.5f * H) * C.s, sx = (px + 0.5f - 0.5f * W) * C.s;
    f3 bc, bX, bY, bZ, bh;
    base_box(bc, bX, bY, bZ, bh);
    float boxc[1][16];
    box_consts(C, bc, bX, bY, bZ, bh, 1.f, boxc[0]);
    const f3 col = mk(0.8f, 0.8f, 0.8f);
    const unsigned rgb = pack_rgb(shade_pixel(C, boxc, &col, 1, -1, sx, sy, default_shade()));
    P.img_bg[3 * (size_t)pix + 0] = (unsigned char)rgb;
    P.img_bg[3 * (size_t)pix + 1] = (unsigned char)(rgb >> 8);
    P.img_bg[3 * (size_t)pix + 2] = (unsigned char)(rgb >> 16);
}

#endif

// OR of a value over lanes 0 .. 15 (the primitives live in lanes 0 .. NPRIM-1): four row_shr DPP steps, the result is read from lane 15
[[maybe_unused]] DEV unsigned or_row0(unsigned x) {
    x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true);   // row_shr:1
    x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true);   // row_shr:2
    x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true);   // row_shr:4
    x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true);   // row_shr:8
    return (unsigned)__builtin_amdgcn_readlane((int)x, 15);
}

// the optional arguments of the frame kernel behind the cameras (a parameter pack: nothing, LcrPlanes, LcrLook, or LcrLook and LcrPlanes): the one of type T, or an empty T
template <typename T>
[[maybe_unused]] DEV T pack_arg() { return T{}; }
template <typename T, typename A, typename... R>
[[maybe_unused]] DEV T pack_arg(const A &a, const R &...r) {
    if constexpr (std::is_same<T, A>::value) return a;
    else return pack_arg<T>(r...);
}
template <typename T, typename... A>
constexpr bool pack_has() { return (std::is_same<T, A>::value || ... || false); }

// LOOK builds: the env's colours over what build_scene drew -- the arm in the variant's colours, cube, second cube and marker in the env's own
[[maybe_unused]] DEV void apply_look(const LcrLook &LK, const LcrLookVar &V, int env, int n, int task, int has_target, f3 *bcol) {
    const f3 arm = mk(V.arm_rgb[0], V.arm_rgb[1], V.arm_rgb[2]), finger = mk(V.finger_rgb[0], V.finger_rgb[1], V.finger_rgb[2]);
    for (int i = 0; i < NARM; i++) bcol[i] = i >= 5 ? finger : arm;
    const float *c = LK.rgb + env;
    int nb = NARM;
    bcol[nb++] = mk(c[0], c[n], c[2 * (size_t)n]);
    if (task == 4) bcol[nb++] = mk(c[3 * (size_t)n], c[4 * (size_t)n], c[5 * (size_t)n]);
    if (has_target) bcol[nb] = mk(c[6 * (size_t)n], c[7 * (size_t)n], c[8 * (size_t)n]);
}

// COUNT: diagnostics build (LCR_RENDER_COUNT=1 and lcr_config.diagnostics): ray-cast passes / primitive tests / pixels written per env into
// active_count / choice / max_sweeps (tools/render_work.py)
// Six waves per SIMD: the 80 registers that takes spill six values of the scene set-up (the chain of link frames), none in the band loop (measured, 32 768 envs:
// 5 waves 2.88 ms, 6: 2.77, 7: 2.92, 8: 2.95; the rounds 1-4 structure with its background prefetch in registers ran 4).
//
// The frame size: TW x TH when they are given (320 x 240, the default: every extent a compile-time constant, the staging rows a static array), else P.img_w x P.img_h
// (lcr_config.image_width / image_height: multiples of 4 in [16, 512]) with the staging rows in dynamic LDS (4 waves x 12 W bytes: six workgroups per CU fit up to
// 320 wide, five at 512 -- the NV = 6 build is compiled for five waves per SIMD).  NV = 16-B vectors of a band (3 W / 4 of them) a lane carries, ceil(3 W / 256).
// EPW = envs per workgroup (1, 2, 4), the mapping for small frames: 4 / EPW waves per env -- 4: two per camera, alternate bands; 2: one per camera; 1: one wave draws
// both frames of its env -- so that the scene set-up of EPW envs runs side by side and a workgroup lives EPW times longer against its launch.
//
// PLANES (a kernel argument of type LcrPlanes is given -- `PLS` is empty, LcrPlanes, LcrLook or both, so the colour-only builds keep their signature; run-time sizes only): the enabled
// depth / segmentation planes of PL are drawn beside the colours.  A band no silhouette touches copies the cached background bands (16 W B of depth, 4 W B of segmentation)
// with 16-B stores.  In a touched band the segmentation band is staged in LDS behind the colours (4 W B more per wave) and leaves as 16-B stores; the depth band is NOT
// staged -- 16 W B per wave would more than double the workgroup's LDS and leave three of the six workgroups of a CU at 320 wide -- but leaves straight from registers: the
// ray-cast tiles store their 16 x 4 floats (64 B per row), the 16-B vectors of every other tile are copied from the background.  No byte of a plane is written twice.
//
// LOOK (a kernel argument of type LcrLook is given; run-time sizes only; include/lcr.h: lcr_enable_look): the env's variant index is wave-uniform.  Through it come the two cameras
// (build_prim receives them: the culling records and boxc stay per camera as they are), the light (one 15-float load per wave and camera, read back into scalar registers) and the
// cached background the untouched bands are copied from -- still plain 16-B copies, from one of K pairs -- and, with PLANES, the background planes of that variant's cameras.  The
// colours of the boxes are replaced right after build_scene (apply_look).  Same expressions as the builds without a look, with values where the constants were: the default variant
// with the task's colours draws the very bytes.
template <bool COUNT, int NV, int EPW, int TW, int TH, typename... PLS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NV > 4 ? 5 : 6, NV > 4 ? 5 : 6))) void lcr_render_obs_kernel(LcrDev P, LcrCam front, LcrCam top, PLS... pls) {
    constexpr bool PLANES = pack_has<LcrPlanes, PLS...>(), LOOK = pack_has<LcrLook, PLS...>();
    const LcrPlanes PL = pack_arg<LcrPlanes>(pls...);
    [[maybe_unused]] const LcrLook LK = pack_arg<LcrLook>(pls...);
    // A workgroup owns EPW envs (one: 2 H rows, front frame then top frame); a wave handles one BAND of 4 rows at a time (12 W B = 3 W / 4 lanes x
    // 16 B; 3 840 B = 240 lanes at 320 wide).  The band starts as a copy of the cached background band (L2 hit); if no primitive's silhouette touches
    // it (wave-uniform) it leaves straight away as non-temporal 16-B stores.  Otherwise the band is
    // staged in LDS, its 16 x 4-pixel tiles that a silhouette touches are ray-cast and
    // overwrite their bytes, and the band is stored from LDS.  No software prefetch across bands and the culling records in LDS rather than in
    // registers: both buy occupancy (six waves per SIMD), which is what hides the L2 latency of the background rows and keeps the store queue fed while
    // other waves ray-cast.
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    constexpr bool FIXED = TW != 0;
    static_assert(!FIXED || (TW % 16 == 0 && TH % 4 == 0 && (3 * TW / 4 + 63) / 64 == NV), "a fixed size has whole tile columns and its own NV");
    static_assert(EPW == 1 || EPW == 2 || EPW == 4, "1, 2 or 4 waves per env");
    static_assert(!(PLANES || LOOK) || (!FIXED && !COUNT), "the planes and look builds take their size at run time and count nothing");
    const int W = FIXED ? TW : P.img_w, H = FIXED ? TH : P.img_h;
    const int NT = (W + 15) >> 4;   // 16-pixel tile columns, the last one partial when W % 16 != 0 (<= 32: one mask word)
    const int VB = 3 * W / 4;       // 16-B vectors of a band
    const int RB = 3 * W;           // bytes of a row
    static_assert(NPRIM <= 16, "one primitive per lane of a DPP row");
    __shared__ Scene S_[EPW];
    __shared__ __attribute__((aligned(16))) unsigned char stage_fixed[FIXED ? 4 * 12 * TW : 16];
    extern __shared__ __attribute__((aligned(16))) unsigned char stage_dyn[];   // [4][12 W] when the size is a run-time value (PLANES: [4][12 W + 4 W], colours then segmentation)
    constexpr int WPE = 4 / EPW;   // waves per env
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int e = wave / WPE, wsub = wave % WPE;
    const int env = blockIdx.x * EPW + e;
    const bool live = env < P.n;   // (a ragged batch: the waves of the missing envs only keep the barriers company)
    Scene &S = S_[e];
    const int tl = EPW == 1 ? (int)threadIdx.x : (int)threadIdx.x & (64 * WPE - 1);   // thread within its env's waves
    // LOOK: the env's variant (wave-uniform: its cameras, light and background) and colours
    [[maybe_unused]] const LcrLookVar *LV = nullptr;
    [[maybe_unused]] int variant = 0;
    if (LOOK && live) { variant = __builtin_amdgcn_readfirstlane(LK.variant[env]); LV = LK.var + variant; }
    if (tl == 0 && live) {
        build_scene(P, env, S);
        if (LOOK) apply_look(LK, *LV, env, P.n, P.task, P.has_target, S.bcol);
    }
    __syncthreads();
    if (tl < 2 * NPRIM && live) {
        const int cam_id = tl / NPRIM, prim = tl - cam_id * NPRIM;
        build_prim(LOOK ? LV->cam[cam_id] : (cam_id ? top : front), cam_id, W, H, S, prim);
    }
    __syncthreads();
    if (!live) return;
    const size_t img_bytes = (size_t)H * W * 3;
    unsigned char *st = FIXED ? stage_fixed + wave * (12 * TW) : stage_dyn + wave * (PLANES ? 16 * W : 4 * RB);
    unsigned char *sgst = st + 4 * RB;   // PLANES: the staged segmentation band
    const int VS = W >> 2;               // PLANES: 16-B vectors of a segmentation band = of one row of a depth band (W of them)
    const int marker = __builtin_amdgcn_readfirstlane(S.marker);
    // co-resident workgroups start at different bands (hashed phase) so that their ray-cast (VALU-bound) and copy
    // (memory-bound) stretches overlap instead of all waves of a SIMD hitting the arm's rows together
    const int NB = H / 4;
    const int rot = (int)(((unsigned)env * 0x9E3779B1u) >> 29) * (2 * NB / 15);   // eight phases, 0 .. 7 (2 NB / 15) < NB  (NB = 60: steps of 8 bands)
    const int tx = lane & 15, ty = lane >> 4;   // pixel of this lane inside a 16 x 4 tile
    // four waves per env: waves 0,1 render camera_front (even / odd bands), waves 2,3 camera_top; two: one camera each; one: both cameras in turn.
    // Everything camera-dependent is wave-uniform
    constexpr int CAM_STEP = WPE >= 2 ? 2 : 1, BAND_STEP = WPE == 4 ? 2 : 1;
    int cam = WPE == 4 ? wsub >> 1 : (WPE == 2 ? wsub : 0);
    do {
    // LOOK: the variant's camera and light, one load per wave and camera (lanes 0 .. 12 the camera, 13 / 14 ambient / diffuse), then wave-uniform values
    [[maybe_unused]] LcrCam CL;
    float amb = 0.3f, dif = 0.6f;
    if (LOOK) {
        const float *vf = reinterpret_cast<const float *>(LV);
        const float w = vf[lane < 13 ? 13 * cam + lane : (lane < 15 ? 13 + lane : 0)];
        auto rl = [&](int i) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), i)); };
        CL.px = rl(0); CL.py = rl(1); CL.pz = rl(2);
        CL.xx = rl(3); CL.xy = rl(4); CL.xz = rl(5); CL.yx = rl(6); CL.yy = rl(7); CL.yz = rl(8); CL.zx = rl(9); CL.zy = rl(10); CL.zz = rl(11);
        CL.s = rl(12); amb = rl(13); dif = rl(14);
    }
    const LcrCam &C = LOOK ? CL : (cam ? top : front);
    const f3 ro = mk(C.px, C.py, C.pz), CX = mk(C.xx, C.xy, C.xz), CY = mk(C.yx, C.yy, C.yz), CZ = mk(C.zx, C.zy, C.zz);
    // culling: one primitive per lane (lane k <-> primitive k).  Per band, every lane computes the pixel interval [xa, xb] its primitive can cover on the
    // band's 4 rows (arm boxes: 2D stadium silhouette, the other boxes: bounding box) -> the interval [ta, tb] of 16-pixel tile columns it touches.
    const float *cull = S.cull[cam][lane < NPRIM ? lane : 0];
    const int bgi = LOOK ? 2 * variant + cam : cam;   // which cached background: one pair per variant
    const u32x4 *bg = reinterpret_cast<const u32x4 *>(LOOK ? LK.bg : P.img_bg) + (size_t)bgi * NB * VB;
    u32x4 *out = reinterpret_cast<u32x4 *>((cam ? P.img_top : P.img_front) + (size_t)env * img_bytes);
    // PLANES: this camera's planes of this env, and their background (null pointer: plane not enabled -- wave-uniform)
    const size_t plane_px = (size_t)H * W;
    f32x4 *dplane = nullptr;
    u32x4 *splane = nullptr;
    const f32x4 *dbg = nullptr;
    const u32x4 *sbg = nullptr;
    if (PLANES) {
        float *dp = cam ? PL.depth_top : PL.depth_front;
        unsigned char *sp = cam ? PL.seg_top : PL.seg_front;
        if (dp) { dplane = reinterpret_cast<f32x4 *>(dp + (size_t)env * plane_px); dbg = reinterpret_cast<const f32x4 *>(PL.bg_depth + (size_t)bgi * plane_px); }
        if (sp) { splane = reinterpret_cast<u32x4 *>(sp + (size_t)env * plane_px); sbg = reinterpret_cast<const u32x4 *>(PL.bg_seg + (size_t)bgi * plane_px); }
    }
    // the depth band b (W vectors: 4 rows of W / 4) without the vectors of the tile columns in `skip` (a tile column = 4 vectors of each row)
    auto copy_depth_band = [&](int b, unsigned skip) {
        const f32x4 *s4 = dbg + (size_t)b * W;
        f32x4 *d4 = dplane + (size_t)b * W;
        for (int i = lane; i < W; i += 64) {
            const int r = (i >= VS) + (i >= 2 * VS) + (i >= 3 * VS);
            if (!((skip >> ((i - r * VS) >> 2)) & 1u)) __builtin_nontemporal_store(s4[i], d4 + i);
        }
    };
    for (int it = WPE == 4 ? wsub & 1 : 0; it < NB; it += BAND_STEP) {
        const int b = it + rot >= NB ? it + rot - NB : it + rot;
        u32x4 *dst = out + b * VB;
        const u32x4 *src = bg + b * VB;
        // a band = VB vectors = NV wave loads, the last one partial (320 wide: 240 = 3 full ones + 48 lanes); in flight while the band is culled
        u32x4 v[NV];
#pragma unroll
        for (int j = 0; j < NV; j++) v[j] = src[min(64 * j + lane, VB - 1)];
        const int row0 = 4 * b;
        const f32x4 cb = *reinterpret_cast<const f32x4 *>(cull);   // y0 y1 x0 x1
        // (the base alone does not make a band worth ray-casting: it is in the background already)
        const bool in_band = lane < NPRIM && (float)(row0 + 3) >= cb.x && (float)row0 <= cb.y;
        int ta = 1 << 20, tb = -1;   // tile columns this lane's primitive can touch on rows row0 .. row0+3 (empty: ta > tb)
        if (in_band) {
            float xa = cb.z, xb = cb.w;
            if (lane < NARM) {
                const f32x4 cs = *reinterpret_cast<const f32x4 *>(cull + 4), ct = *reinterpret_cast<const f32x4 *>(cull + 8);
                const float au = cs.x, av = cs.y, du = cs.z, R = cs.w, slope = ct.x, inv_dv = ct.y, strip_hw = ct.z;
                const bool flat = ct.w != 0.f;
                const float f0 = (float)row0 - R - av, f1 = (float)(row0 + 3) + R - av;
                const float sA = f0 * inv_dv, sB = f1 * inv_dv;
                const float s0 = flat ? 0.f : clampf(fminf(sA, sB), 0.f, 1.f), s1 = flat ? 1.f : clampf(fmaxf(sA, sB), 0.f, 1.f);
                const float e0 = s0 * du, e1 = s1 * du;
                const float c0 = fmaf((float)row0 - av, slope, au), c1 = fmaf((float)(row0 + 3) - av, slope, au);
                xa = fmaxf(fmaxf(au + fminf(e0, e1) - R, fminf(c0, c1) - strip_hw), xa);
                xb = fminf(fminf(au + fmaxf(e0, e1) + R, fmaxf(c0, c1) + strip_hw), xb);
            }
            if (xb >= 0.f && xa <= (float)(W - 1) && xa <= xb) {
                ta = (int)fmaxf(xa * (1.f / 16.f), 0.f); tb = (int)fminf(xb * (1.f / 16.f), (float)(NT - 1));
            }
        }
        // tile columns of the band that a primitive other than the base touches
        unsigned U = 0u;
        if (__any(ta <= tb && lane != BASE)) U = or_row0(ta <= tb && lane != BASE ? (2u << tb) - (1u << ta) : 0u);
        if (U == 0u) {
#pragma unroll
            for (int j = 0; j < NV; j++)
                if (64 * j + lane < VB) __builtin_nontemporal_store(v[j], dst + 64 * j + lane);
            if (PLANES) {
                if (dplane) copy_depth_band(b, 0u);
                if (splane)
                    for (int i = lane; i < VS; i += 64) __builtin_nontemporal_store(sbg[(size_t)b * VS + i], splane + (size_t)b * VS + i);
            }
            continue;
        }
        const unsigned U0 = U;
        if (PLANES && splane) {
            u32x4 *sgv = reinterpret_cast<u32x4 *>(sgst);
            for (int i = lane; i < VS; i += 64) sgv[i] = sbg[(size_t)b * VS + i];
        }
        u32x4 *sv = reinterpret_cast<u32x4 *>(st);
#pragma unroll
        for (int j = 0; j < NV; j++)
            if (64 * j + lane < VB) sv[64 * j + lane] = v[j];
        // rays of this lane's tile row: d(px) = -Z + sy Y + sx(px) X, camera looks along -Z
        const float sy = -((float)(row0 + ty) + 0.5f - 0.5f * H) * C.s;
        const f3 rbase = axpy(sy, CY, neg(CZ));
        for (; U; U &= U - 1u) {
            const int t = __builtin_ctz(U);
            const unsigned m = (unsigned)__ballot(ta <= t && tb >= t);
            // (a partial last tile column: lanes beyond the row's end follow the wave with the row's last pixel and write nothing)
            const int pxt = 16 * t + tx, px = FIXED ? pxt : min(pxt, W - 1);
            const float sx = ((float)px + 0.5f - 0.5f * W) * C.s;
            const f3 rdu = axpy(sx, CX, rbase);
            unsigned char *stpx = st + ty * RB + 3 * px;
            unsigned rgb = 0u;
            float tnear = 0.f;
            int knear = -1;
            bool mhit = false;
            const bool wrote = shade_span<PLANES>(S, cam, marker, ro, sx, sy, rdu, m, stpx, rgb, tnear, knear, mhit, amb, dif) && (FIXED || pxt < W);
            if (PLANES && pxt < W) {   // every pixel of a ray-cast tile: `m` holds all that can be seen in it, the base included
                if (dplane) __builtin_nontemporal_store(fminf(tnear, PL.far), reinterpret_cast<float *>(dplane) + (size_t)(row0 + ty) * W + px);
                if (splane) {
                    const unsigned id = knear >= 0 ? (unsigned)knear + 2u : (rdu.z * rsq(dot(rdu, rdu)) < -1e-6f ? 1u : 0u);   // (the horizon rule of the background colours)
                    sgst[ty * W + px] = (unsigned char)(id | (mhit ? 0x80u : 0u));
                }
            }
            if (wrote) {
                stpx[0] = (unsigned char)rgb;
                stpx[1] = (unsigned char)(rgb >> 8);
                stpx[2] = (unsigned char)(rgb >> 16);
            }
            if (COUNT && P.active_count) {
                const int nw = __popcll(__ballot(wrote));
                if (lane == 0) { atomicAdd(&P.active_count[env], 1u); atomicAdd(&P.choice[env], (unsigned)__popc(m)); atomicAdd(&P.max_sweeps[env], (unsigned)nw); }
            }
        }
#pragma unroll
        for (int j = 0; j < NV; j++)
            if (64 * j + lane < VB) __builtin_nontemporal_store(sv[64 * j + lane], dst + 64 * j + lane);
        if (PLANES) {
            if (dplane) copy_depth_band(b, U0);
            if (splane) {
                const u32x4 *sgv = reinterpret_cast<const u32x4 *>(sgst);
                for (int i = lane; i < VS; i += 64) __builtin_nontemporal_store(sgv[i], splane + (size_t)b * VS + i);
            }
        }
    }
    } while ((cam += CAM_STEP) < 2);
}

#if LCR_RENDER_PLANES || LCR_RENDER_LOOK
// one pixel, every primitive of the scene: the nearest opaque surface -- t along the un-normalised ray, which is metres along the optical axis (1e30: sky) -- and the
// segmentation byte of include/lcr.h
DEV void trace_pixel(const LcrCam &C, const float (*boxc)[16], int nbox, int marker, float sx, float sy, float &t, unsigned &seg) {
    const f3 ro = mk(C.px, C.py, C.pz);
    const f3 d = mk(C.xx * sx + C.yx * sy - C.zx, C.xy * sx + C.yy * sy - C.zy, C.xz * sx + C.yz * sy - C.zz);
    const bool down = d.z * rsq(dot(d, d)) < -1e-6f;   // the horizon rule of floor_or_sky
    float tbest = down ? -ro.z * rcp(d.z) : 1e30f;
    int kbest = -1;
    bool mhit = false;
    for (int k = 0; k < nbox; k++) {
        float tmin, ld;
        if (!box_hit(boxc[k], sx, sy, tbest, tmin, ld)) continue;
        if (k == marker) mhit = true;   // (the marker is the last box: every opaque primitive has been seen)
        else { tbest = tmin; kbest = k; }
    }
    t = tbest;
    seg = (kbest >= 0 ? (unsigned)kbest + 2u : (down ? 1u : 0u)) | (mhit ? 0x80u : 0u);
}
#endif

#if LCR_RENDER_PLANES

// the background planes of the two observation cameras (floor, sky, the arm's base), rendered once at lcr_enable_image_planes into PL.bg_depth / PL.bg_seg ([2][H][W])
__global__ __launch_bounds__(256) void lcr_render_bg_planes_kernel(LcrDev P, LcrCam front, LcrCam top, LcrPlanes PL) {
    const int W = P.img_w, H = P.img_h;
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= 2 * W * H) return;
    const bool is_top = pix >= W * H;
    const int p = is_top ? pix - W * H : pix;
    const int row = p / W, px = p - row * W;
    const LcrCam &C = is_top ? top : front;
    const float sy = -(row + 0.5f - 0.5f * H) * C.s, sx = (px + 0.5f - 0.5f * W) * C.s;
    f3 bc, bX, bY, bZ, bh;
    base_box(bc, bX, bY, bZ, bh);
    float boxc[1][16];
    box_consts(C, bc, bX, bY, bZ, bh, 1.f, boxc[0]);
    float t;
    unsigned seg;
    trace_pixel(C, boxc, 1, -1, sx, sy, t, seg);
    PL.bg_depth[pix] = fminf(t, PL.far);
    PL.bg_seg[pix] = (unsigned char)seg;
}

// one env, arbitrary camera / resolution, one thread per pixel, no culling, no cached background: the sibling of lcr_render_single_kernel.  Either output may be null
__global__ __launch_bounds__(256) void lcr_render_single_planes_kernel(LcrDev P, LcrCam cam, int env, int W, int H, float far, float *depth, unsigned char *seg_out) {
    __shared__ Scene S;
    if (threadIdx.x == 0) build_scene(P, env, S);
    __syncthreads();
    if (threadIdx.x < NBOX && (int)threadIdx.x < S.nbox)
        box_consts(cam, S.bc[threadIdx.x], S.bX[threadIdx.x], S.bY[threadIdx.x], S.bZ[threadIdx.x], S.bh[threadIdx.x], S.balpha[threadIdx.x], S.boxc[0][threadIdx.x]);
    __syncthreads();
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= W * H) return;
    const int v = pix / W, u = pix - v * W;
    const float sx = (u + 0.5f - 0.5f * W) * cam.s, sy = -(v + 0.5f - 0.5f * H) * cam.s;
    float t;
    unsigned seg;
    trace_pixel(cam, S.boxc[0], S.nbox, S.marker, sx, sy, t, seg);
    if (depth) depth[pix] = fminf(t, far);
    if (seg_out) seg_out[pix] = (unsigned char)seg;
}
#endif

#if LCR_RENDER_SMALL
// one env, arbitrary camera / resolution (render(), 640x640 camera_vizu): one thread per pixel, no culling, no cached background
__global__ __launch_bounds__(256) void lcr_render_single_kernel(LcrDev P, LcrCam cam, int env, int W, int H, unsigned char *out) {
    __shared__ Scene S;
    if (threadIdx.x == 0) build_scene(P, env, S);
    __syncthreads();
    if (threadIdx.x < NBOX && (int)threadIdx.x < S.nbox)
        box_consts(cam, S.bc[threadIdx.x], S.bX[threadIdx.x], S.bY[threadIdx.x], S.bZ[threadIdx.x], S.bh[threadIdx.x], S.balpha[threadIdx.x], S.boxc[0][threadIdx.x]);
    __syncthreads();
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= W * H) return;
    const int v = pix / W, u = pix - v * W;
    const float sx = (u + 0.5f - 0.5f * W) * cam.s, sy = -(v + 0.5f - 0.5f * H) * cam.s;
    const unsigned rgb = pack_rgb(shade_pixel(cam, S.boxc[0], S.bcol, S.nbox, S.marker, sx, sy, default_shade()));
    out[3 * (size_t)pix + 0] = (unsigned char)rgb;
    out[3 * (size_t)pix + 1] = (unsigned char)(rgb >> 8);
    out[3 * (size_t)pix + 2] = (unsigned char)(rgb >> 16);
}

// terminal poses of the listed envs (the step kernel has already reset them: term_obs / term_quat hold the last pose of the episode) gathered into a
// compact [nq][count] qpos + [3][count] target block, so that lcr_render_obs_kernel can draw their last frames as one batch (lcr_render_terminal)
__global__ __launch_bounds__(256) void lcr_gather_terminal_kernel(LcrDev P, const int *ids, int count, float *qpos_out, float *target_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const size_t N = (size_t)P.n, C = (size_t)count;
    const int e = ids[i];
    const float *t = P.term_obs + e, *tq = P.term_quat + e;   // term_obs rows: arm_qpos 0-5, arm_qvel 6-11, cube 12-14, aux 15-17
    for (int j = 0; j < 6; j++) qpos_out[j * C + i] = t[j * N];
    for (int j = 0; j < 3; j++) qpos_out[(6 + j) * C + i] = t[(12 + j) * N];
    for (int j = 0; j < 4; j++) qpos_out[(9 + j) * C + i] = tq[j * N];
    if (P.task == 4) {
        for (int j = 0; j < 3; j++) qpos_out[(13 + j) * C + i] = t[(15 + j) * N];
        for (int j = 0; j < 4; j++) qpos_out[(16 + j) * C + i] = tq[(4 + j) * N];
    }
    for (int j = 0; j < 3; j++) target_out[j * C + i] = P.has_target ? t[(15 + j) * N] : 0.f;
}

#endif

#if LCR_RENDER_LOOK
// ---- the look (include/lcr.h: lcr_enable_look) ----
// the cached backgrounds of the K variants, LK.bg [K][2][H][W][3]: lcr_render_bg_kernel with each variant's cameras, colours and light
__global__ __launch_bounds__(256) void lcr_render_bg_look_kernel(LcrDev P, LcrLook LK, int K) {
    const int W = P.img_w, H = P.img_h, per = 2 * W * H;
    const int gpix = blockIdx.x * blockDim.x + threadIdx.x;   // (K <= 64 pairs of at most 512 x 512: below 2^26)
    if (gpix >= K * per) return;
    const int k = gpix / per, pix = gpix - k * per;
    const LcrLookVar &V = LK.var[k];
    const bool is_top = pix >= W * H;
    const int p = is_top ? pix - W * H : pix;
    const int row = p / W, px = p - row * W;
    const LcrCam C = V.cam[is_top ? 1 : 0];
    const float sy = -(row + 0.5f - 0.5f * H) * C.s, sx = (px + 0.5f - 0.5f * W) * C.s;
    f3 bc, bX, bY, bZ, bh;
    base_box(bc, bX, bY, bZ, bh);
    float boxc[1][16];
    box_consts(C, bc, bX, bY, bZ, bh, 1.f, boxc[0]);
    const f3 col = mk(V.arm_rgb[0], V.arm_rgb[1], V.arm_rgb[2]);
    const unsigned rgb = pack_rgb(shade_pixel(C, boxc, &col, 1, -1, sx, sy, look_shade(V)));
    unsigned char *o = const_cast<unsigned char *>(LK.bg) + 3 * (size_t)gpix;
    o[0] = (unsigned char)rgb; o[1] = (unsigned char)(rgb >> 8); o[2] = (unsigned char)(rgb >> 16);
}

// their planes, PL.bg_depth / PL.bg_seg [K][2][H][W]
__global__ __launch_bounds__(256) void lcr_render_bg_planes_look_kernel(LcrDev P, LcrLook LK, int K, LcrPlanes PL) {
    const int W = P.img_w, H = P.img_h, per = 2 * W * H;
    const int gpix = blockIdx.x * blockDim.x + threadIdx.x;
    if (gpix >= K * per) return;
    const int k = gpix / per, pix = gpix - k * per;
    const bool is_top = pix >= W * H;
    const int p = is_top ? pix - W * H : pix;
    const int row = p / W, px = p - row * W;
    const LcrCam C = LK.var[k].cam[is_top ? 1 : 0];
    const float sy = -(row + 0.5f - 0.5f * H) * C.s, sx = (px + 0.5f - 0.5f * W) * C.s;
    f3 bc, bX, bY, bZ, bh;
    base_box(bc, bX, bY, bZ, bh);
    float boxc[1][16];
    box_consts(C, bc, bX, bY, bZ, bh, 1.f, boxc[0]);
    float t;
    unsigned seg;
    trace_pixel(C, boxc, 1, -1, sx, sy, t, seg);
    PL.bg_depth[gpix] = fminf(t, PL.far);
    PL.bg_seg[gpix] = (unsigned char)seg;
}

// lcr_render_single_kernel with the look of env `look_env` of LK (its variant's colours and light, its own colours); the camera is the caller's
__global__ __launch_bounds__(256) void lcr_render_single_look_kernel(LcrDev P, LcrCam cam, int env, int W, int H, unsigned char *out, LcrLook LK, int look_env, int look_n) {
    __shared__ Scene S;
    const LcrLookVar &V = LK.var[LK.variant[look_env]];
    if (threadIdx.x == 0) {
        build_scene(P, env, S);
        apply_look(LK, V, look_env, look_n, P.task, P.has_target, S.bcol);
    }
    __syncthreads();
    if (threadIdx.x < NBOX && (int)threadIdx.x < S.nbox)
        box_consts(cam, S.bc[threadIdx.x], S.bX[threadIdx.x], S.bY[threadIdx.x], S.bZ[threadIdx.x], S.bh[threadIdx.x], S.balpha[threadIdx.x], S.boxc[0][threadIdx.x]);
    __syncthreads();
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= W * H) return;
    const int v = pix / W, u = pix - v * W;
    const float sx = (u + 0.5f - 0.5f * W) * cam.s, sy = -(v + 0.5f - 0.5f * H) * cam.s;
    const unsigned rgb = pack_rgb(shade_pixel(cam, S.boxc[0], S.bcol, S.nbox, S.marker, sx, sy, look_shade(V)));
    out[3 * (size_t)pix + 0] = (unsigned char)rgb;
    out[3 * (size_t)pix + 1] = (unsigned char)(rgb >> 8);
    out[3 * (size_t)pix + 2] = (unsigned char)(rgb >> 16);
}

// Philox-4x32-10 (the generator of lcr_fill_random_actions): key = seed, counter = (global env id, episode, block)
DEV void look_philox(unsigned long long seed, unsigned long long gid, uint32_t episode, uint32_t blk, uint32_t (&c)[4]) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    c[0] = (uint32_t)gid; c[1] = (uint32_t)(gid >> 32); c[2] = episode; c[3] = blk;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0], hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// The look of the envs that were reset (include/lcr.h: the sampler).  `cur` / `term`: [10][n] words, row 0 the variant, rows 1 .. 9 the colours (float bits).
// mode 0: envs with flag[e] != 0 (flag null: all) hand their look to `term` (when given), count an episode and -- with a sampler -- draw that episode's look;
// mode 1: every env draws the look of episode 0 (lcr_enable_look)
__global__ __launch_bounds__(256) void lcr_look_redraw_kernel(int n, long long env_off, const unsigned char *flag, int mode, LcrLookSampler SM, int *cur, unsigned *episode, int *term) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    uint32_t ep = 0;
    if (mode == 0) {
        if (flag && !flag[e]) return;
        if (term)
            for (int j = 0; j < 10; j++) term[(size_t)j * n + e] = cur[(size_t)j * n + e];
        ep = episode[e] + 1u;
        episode[e] = ep;
    }
    if (!SM.on) return;
    const unsigned long long gid = (unsigned long long)(env_off + e);
    uint32_t w[12];
    for (uint32_t b = 0; b < 3; b++) {
        uint32_t c[4];
        look_philox(SM.seed, gid, ep, b, c);
        for (int i = 0; i < 4; i++) w[4 * b + i] = c[i];
    }
    cur[e] = (int)__umulhi(w[0], (uint32_t)SM.K);
    for (int j = 0; j < 9; j++) {
        const float u = (float)(w[1 + j] >> 8) * (1.0f / 16777216.0f);
        cur[(size_t)(1 + j) * n + e] = __float_as_int(fminf(fmaf(u, SM.rng[j], SM.lo[j]), SM.hi[j]));
    }
}

// the looks of the listed envs as a compact [10][count] block (lcr_render_terminal: the terminal looks)
__global__ __launch_bounds__(256) void lcr_look_gather_kernel(const int *ids, int count, int n, const int *look, int *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int e = ids[i];
    for (int j = 0; j < 10; j++) out[(size_t)j * count + i] = look[(size_t)j * n + e];
}
#endif

#if LCR_RENDER_WRIST
// ---- the wrist camera (include/lcr.h: lcr_enable_wrist_camera) ----
// A camera that rides on a link moves every step: it has no cached background.  Every 16 x 4 tile is shaded, floor or sky per pixel in registers, and only the boxes of the
// tile's wave-uniform mask are tested.  A dedicated kernel: lcr_render_obs_kernel, its register budget and its bytes stay as they are.

// the chain of link frames build_scene places the arm's boxes with (build_scene itself, shared with the two-camera kernels, stays as it is: exposing its frames moved their
// register allocation)
DEV void wrist_frames(const LcrDev &P, int env, ArmFrames &F) {
    float q[6];
    for (int j = 0; j < 6; j++) q[j] = P.qpos[(size_t)j * P.n + env];
    arm_frames(q, F);
}

// (wrist_camera, the world pose of the mounted camera from that chain, lives in lcr_wrist_pose.h: the point-cloud kernel computes the same pose with the same code)

// one pixel of the wrist camera, the boxes of mask `m` (uniform; the marker is the last box): linear rgb, t of the nearest opaque surface along the un-normalised ray
// (1e30: sky) and the segmentation byte.  The expressions of shade_pixel / trace_pixel, with the floor rule a camera on a link needs: the floor is seen only where the
// normalised d.z < -1e-6 AND the camera is above it -- at or below the floor plane those rays take the sky formula and the floor limits no box (a negative floor parameter
// would hide every box)
DEV void wrist_pixel(const LcrCam &C, const float (*boxc)[16], const f3 *bcol, unsigned m, int marker, float sx, float sy, const Shade &h, f3 &out, float &tnear, unsigned &seg) {
    const f3 ro = mk(C.px, C.py, C.pz);
    const f3 d = mk(C.xx * sx + C.yx * sy - C.zx, C.xy * sx + C.yy * sy - C.zy, C.xz * sx + C.yz * sy - C.zz);
    const float inv_len = rsq(dot(d, d));
    const float rdz = d.z * inv_len;
    const bool floor = rdz < -1e-6f && ro.z > 0.f;
    float tbest = 1e30f;
    if (floor) {   // checker floor, 0.1 m squares, normal +z
        tbest = -ro.z * rcp(d.z);
        const float fx = fmaf(tbest, d.x, ro.x), fy = fmaf(tbest, d.y, ro.y);
        const int cell = ((int)floorf(fx * 10.f) + (int)floorf(fy * 10.f)) & 1;
        const float lam = fminf(fmaf(-h.dif, rdz, h.amb), 1.f);
        out = lam * (cell ? h.floor_odd : h.floor_even);
    } else {
        const float a = clampf(rdz * 2.f, 0.f, 1.f);
        out = mk(h.sky.x + a * h.sky_slope.x, h.sky.y + a * h.sky_slope.y, h.sky.z + a * h.sky_slope.z);
    }
    int kbest = -1;
    float talpha = 0.f, tlamd = 0.f;
    for (unsigned mm = m; mm; mm &= mm - 1u) {
        const int k = __builtin_ctz(mm);
        float tmin, ld;
        if (!box_hit(boxc[k], sx, sy, tbest, tmin, ld)) continue;
        if (k == marker) { tlamd = ld; talpha = boxc[k][15]; }
        else { tbest = tmin; kbest = k; out = fminf(fmaf(h.dif * inv_len, ld, h.amb), 1.f) * bcol[k]; }
    }
    if (talpha > 0.f) out = axpy(talpha * fmaf(h.dif * inv_len, tlamd, h.amb), bcol[marker < 0 ? 0 : marker], (1.f - talpha) * out);
    tnear = tbest;
    seg = (kbest >= 0 ? (unsigned)kbest + 2u : (floor ? 1u : 0u)) | (talpha > 0.f ? 0x80u : 0u);
}

// The batched wrist frames, [n][H][W][3] at the handle's frame size (run-time values), with the planes WR points at (PLANES) and the envs' looks (LOOK: the variant's floor,
// sky, light and arm colours, the env's own colours; the variant's camera offsets belong to the two scene cameras).  The mapping of lcr_render_obs_kernel: a workgroup draws
// EPW envs (1, 2, 4) with 4 / EPW waves each, a wave owns bands of 4 rows in turn; thread 0 of an env builds the scene and the camera, one thread per primitive its
// culling record (build_prim: a primitive that crosses the plane 0.02 m in front of the camera -- the mounting link's own box usually does -- gets the full-frame record).
// The band's bytes are staged in LDS (12 W B of colours, PLANES: 4 W B of segmentation behind them) and leave as non-temporal 16-B stores; the depth band goes straight
// from registers, 64 B per tile row.
template <bool PLANES, bool LOOK, int EPW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6, 6))) void lcr_render_wrist_kernel(LcrDev P, LcrWrist WR, LcrLook LK) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    static_assert(EPW == 1 || EPW == 2 || EPW == 4, "1, 2 or 4 waves per env");
    static_assert(NPRIM <= 16, "one primitive per lane of a DPP row");
    const int W = P.img_w, H = P.img_h;
    const int NT = (W + 15) >> 4;   // 16-pixel tile columns, the last one partial when W % 16 != 0
    const int VB = 3 * W / 4;       // 16-B vectors of a colour band
    const int RB = 3 * W;           // bytes of a row
    const int VS = W >> 2;          // 16-B vectors of a segmentation band
    const int NB = H / 4;
    __shared__ Scene S_[EPW];
    __shared__ LcrCam C_[EPW];
    extern __shared__ __attribute__((aligned(16))) unsigned char stage_dyn[];   // [4][12 W] (PLANES: [4][12 W + 4 W], colours then segmentation)
    constexpr int WPE = 4 / EPW;   // waves per env
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int e = wave / WPE, wsub = wave % WPE;
    const int env = blockIdx.x * EPW + e;
    const bool live = env < P.n;   // (a ragged batch: the waves of the missing envs only keep the barriers company)
    Scene &S = S_[e];
    const int tl = EPW == 1 ? (int)threadIdx.x : (int)threadIdx.x & (64 * WPE - 1);   // thread within its env's waves
    [[maybe_unused]] const LcrLookVar *LV = nullptr;
    if (LOOK && live) LV = LK.var + __builtin_amdgcn_readfirstlane(LK.variant[env]);
    if (tl == 0 && live) {
        ArmFrames F;
        build_scene(P, env, S);
        wrist_frames(P, env, F);
        if (LOOK) apply_look(LK, *LV, env, P.n, P.task, P.has_target, S.bcol);
        wrist_camera(F, WR.mount, C_[e]);
    }
    __syncthreads();
    if (tl < NPRIM && live) build_prim(C_[e], 0, W, H, S, tl);
    __syncthreads();
    if (!live) return;
    // the camera and the light: wave-uniform values
    auto uni = [](float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); };
    LcrCam C;
    C.px = uni(C_[e].px); C.py = uni(C_[e].py); C.pz = uni(C_[e].pz);
    C.xx = uni(C_[e].xx); C.xy = uni(C_[e].xy); C.xz = uni(C_[e].xz); C.yx = uni(C_[e].yx); C.yy = uni(C_[e].yy); C.yz = uni(C_[e].yz);
    C.zx = uni(C_[e].zx); C.zy = uni(C_[e].zy); C.zz = uni(C_[e].zz); C.s = uni(C_[e].s);
    const Shade h = LOOK ? look_shade(*LV) : default_shade();
    unsigned char *st = stage_dyn + wave * (PLANES ? 16 * W : 12 * W);
    unsigned char *sgst = st + 4 * RB;   // PLANES: the staged segmentation band
    const int marker = __builtin_amdgcn_readfirstlane(S.marker);
    const int tx = lane & 15, ty = lane >> 4;   // pixel of this lane inside a 16 x 4 tile
    const float *cull = S.cull[0][lane < NPRIM ? lane : 0];   // culling: one primitive per lane
    const size_t plane_px = (size_t)H * W;
    u32x4 *out = reinterpret_cast<u32x4 *>(WR.img + (size_t)env * plane_px * 3);
    float *dplane = PLANES && WR.depth ? WR.depth + (size_t)env * plane_px : nullptr;
    u32x4 *splane = PLANES && WR.seg ? reinterpret_cast<u32x4 *>(WR.seg + (size_t)env * plane_px) : nullptr;
    for (int b = wsub; b < NB; b += WPE) {
        const int row0 = 4 * b;
        // the tile columns [ta, tb] this lane's primitive can touch on rows row0 .. row0 + 3 (empty: ta > tb): the interval arithmetic of lcr_render_obs_kernel
        const f32x4 cb = *reinterpret_cast<const f32x4 *>(cull);   // y0 y1 x0 x1
        const bool in_band = lane < NPRIM && (float)(row0 + 3) >= cb.x && (float)row0 <= cb.y;
        int ta = 1 << 20, tb = -1;
        if (in_band) {
            float xa = cb.z, xb = cb.w;
            if (lane < NARM) {
                const f32x4 cs = *reinterpret_cast<const f32x4 *>(cull + 4), ct = *reinterpret_cast<const f32x4 *>(cull + 8);
                const float au = cs.x, av = cs.y, du = cs.z, R = cs.w, slope = ct.x, inv_dv = ct.y, strip_hw = ct.z;
                const bool flat = ct.w != 0.f;
                const float f0 = (float)row0 - R - av, f1 = (float)(row0 + 3) + R - av;
                const float sA = f0 * inv_dv, sB = f1 * inv_dv;
                const float s0 = flat ? 0.f : clampf(fminf(sA, sB), 0.f, 1.f), s1 = flat ? 1.f : clampf(fmaxf(sA, sB), 0.f, 1.f);
                const float e0 = s0 * du, e1 = s1 * du;
                const float c0 = fmaf((float)row0 - av, slope, au), c1 = fmaf((float)(row0 + 3) - av, slope, au);
                xa = fmaxf(fmaxf(au + fminf(e0, e1) - R, fminf(c0, c1) - strip_hw), xa);
                xb = fminf(fminf(au + fmaxf(e0, e1) + R, fmaxf(c0, c1) + strip_hw), xb);
            }
            if (xb >= 0.f && xa <= (float)(W - 1) && xa <= xb) {
                ta = (int)fmaxf(xa * (1.f / 16.f), 0.f); tb = (int)fminf(xb * (1.f / 16.f), (float)(NT - 1));
            }
        }
        const float sy = -((float)(row0 + ty) + 0.5f - 0.5f * H) * C.s;
        for (int t = 0; t < NT; t++) {
            const unsigned m = (unsigned)__ballot(ta <= t && tb >= t);   // (lanes beyond the primitives hold an empty interval)
            // (a partial last tile column: lanes beyond the row's end follow the wave with the row's last pixel and write nothing)
            const int pxt = 16 * t + tx, px = min(pxt, W - 1);
            const float sx = ((float)px + 0.5f - 0.5f * W) * C.s;
            f3 col;
            float tnear;
            unsigned seg;
            wrist_pixel(C, S.boxc[0], S.bcol, m, marker, sx, sy, h, col, tnear, seg);
            if (pxt < W) {
                const unsigned rgb = pack_rgb(col);
                unsigned char *stpx = st + ty * RB + 3 * px;
                stpx[0] = (unsigned char)rgb;
                stpx[1] = (unsigned char)(rgb >> 8);
                stpx[2] = (unsigned char)(rgb >> 16);
                if (PLANES) {
                    if (dplane) __builtin_nontemporal_store(fminf(tnear, WR.far), dplane + (size_t)(row0 + ty) * W + px);
                    if (splane) sgst[ty * W + px] = (unsigned char)seg;
                }
            }
        }
        const u32x4 *sv = reinterpret_cast<const u32x4 *>(st);
        for (int i = lane; i < VB; i += 64) __builtin_nontemporal_store(sv[i], out + (size_t)b * VB + i);
        if (PLANES && splane) {
            const u32x4 *sgv = reinterpret_cast<const u32x4 *>(sgst);
            for (int i = lane; i < VS; i += 64) __builtin_nontemporal_store(sgv[i], splane + (size_t)b * VS + i);
        }
    }
}

// one env through the wrist camera at any size, one thread per pixel, no culling: the sibling of lcr_render_single_kernel / lcr_render_single_planes_kernel.  Any of the
// three outputs may be null.  look_env >= 0: with the look of env `look_env` of LK (its variant's colours and light, its own colours)
__global__ __launch_bounds__(256) void lcr_render_single_wrist_kernel(LcrDev P, LcrWristMount M, int env, int W, int H, float far, unsigned char *out, float *depth, unsigned char *seg_out,
                                                                      LcrLook LK, int look_env, int look_n) {
    __shared__ Scene S;
    __shared__ LcrCam C;
    if (threadIdx.x == 0) {
        ArmFrames F;
        build_scene(P, env, S);
        wrist_frames(P, env, F);
        if (look_env >= 0) apply_look(LK, LK.var[LK.variant[look_env]], look_env, look_n, P.task, P.has_target, S.bcol);
        wrist_camera(F, M, C);
    }
    __syncthreads();
    if (threadIdx.x < NBOX && (int)threadIdx.x < S.nbox)
        box_consts(C, S.bc[threadIdx.x], S.bX[threadIdx.x], S.bY[threadIdx.x], S.bZ[threadIdx.x], S.bh[threadIdx.x], S.balpha[threadIdx.x], S.boxc[0][threadIdx.x]);
    __syncthreads();
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= W * H) return;
    const int v = pix / W, u = pix - v * W;
    const float sx = (u + 0.5f - 0.5f * W) * C.s, sy = -(v + 0.5f - 0.5f * H) * C.s;
    const Shade h = look_env >= 0 ? look_shade(LK.var[LK.variant[look_env]]) : default_shade();
    f3 col;
    float t;
    unsigned seg;
    wrist_pixel(C, S.boxc[0], S.bcol, (1u << S.nbox) - 1u, S.marker, sx, sy, h, col, t, seg);
    if (out) {
        const unsigned rgb = pack_rgb(col);
        out[3 * (size_t)pix + 0] = (unsigned char)rgb;
        out[3 * (size_t)pix + 1] = (unsigned char)(rgb >> 8);
        out[3 * (size_t)pix + 2] = (unsigned char)(rgb >> 16);
    }
    if (depth) depth[pix] = fminf(t, far);
    if (seg_out) seg_out[pix] = (unsigned char)seg;
}
#endif

}  // namespace

// the launchers of the run-time sizes live in unit 1
void lcr_launch_render_obs_sized(const LcrDev &P, const LcrCam &front, const LcrCam &top, bool count, void *stream);

namespace {
template <bool COUNT, int NV, int EPW, int TW, int TH>
void launch_obs(const LcrDev &P, const LcrCam &front, const LcrCam &top, void *stream) {
    const size_t lds = TW ? 0 : (size_t)4 * 12 * P.img_w;
    hipLaunchKernelGGL((lcr_render_obs_kernel<COUNT, NV, EPW, TW, TH>), dim3((P.n + EPW - 1) / EPW), dim3(256), lds, (hipStream_t)stream, P, front, top);
}
#if LCR_RENDER_SIZED
template <bool COUNT>
void launch_obs_sized(const LcrDev &P, const LcrCam &front, const LcrCam &top, void *stream) {
    const int W = P.img_w, epw = P.img_epw;
    const int nv = (3 * W / 4 + 63) / 64;   // wave loads of a band: 1 up to 85 px wide, 2 up to 170, 4 up to 341, 6 up to 512
    if (nv > 4) return launch_obs<COUNT, 6, 1, 0, 0>(P, front, top, stream);
    if (nv > 2) return launch_obs<COUNT, 4, 1, 0, 0>(P, front, top, stream);
    if (nv > 1) {
        if (epw == 4) return launch_obs<COUNT, 2, 4, 0, 0>(P, front, top, stream);
        if (epw == 2) return launch_obs<COUNT, 2, 2, 0, 0>(P, front, top, stream);
        return launch_obs<COUNT, 2, 1, 0, 0>(P, front, top, stream);
    }
    if (epw == 4) return launch_obs<COUNT, 1, 4, 0, 0>(P, front, top, stream);
    if (epw == 2) return launch_obs<COUNT, 1, 2, 0, 0>(P, front, top, stream);
    return launch_obs<COUNT, 1, 1, 0, 0>(P, front, top, stream);
}
#endif
}  // namespace

#if LCR_RENDER_SIZED
void lcr_launch_render_obs_sized(const LcrDev &P, const LcrCam &front, const LcrCam &top, bool count, void *stream) {
    if (count) launch_obs_sized<true>(P, front, top, stream);
    else launch_obs_sized<false>(P, front, top, stream);
}
#endif

#if LCR_RENDER_PLANES
namespace {
template <int NV, int EPW>
void launch_obs_planes(const LcrDev &P, const LcrCam &front, const LcrCam &top, const LcrPlanes &PL, void *stream) {
    const size_t lds = (size_t)4 * 16 * P.img_w;   // per wave: 12 W B of colours + 4 W B of segmentation
    hipLaunchKernelGGL((lcr_render_obs_kernel<false, NV, EPW, 0, 0, LcrPlanes>), dim3((P.n + EPW - 1) / EPW), dim3(256), lds, (hipStream_t)stream, P, front, top, PL);
}
}  // namespace

// colour frames + the enabled planes in one launch: the run-time-size builds at every size (320 x 240 included), same mappings as launch_obs_sized
int lcr_launch_render_obs_planes(const LcrDev &P, const LcrCam &front, const LcrCam &top, const LcrPlanes &PL, void *stream) {
    if (!P.img_front || !P.img_top || !PL.bg_depth || !PL.bg_seg) return (int)hipErrorInvalidValue;
    const int nv = (3 * P.img_w / 4 + 63) / 64, epw = P.img_epw;
    if (nv > 4) launch_obs_planes<6, 1>(P, front, top, PL, stream);
    else if (nv > 2) launch_obs_planes<4, 1>(P, front, top, PL, stream);
    else if (nv > 1) {
        if (epw == 4) launch_obs_planes<2, 4>(P, front, top, PL, stream);
        else if (epw == 2) launch_obs_planes<2, 2>(P, front, top, PL, stream);
        else launch_obs_planes<2, 1>(P, front, top, PL, stream);
    } else {
        if (epw == 4) launch_obs_planes<1, 4>(P, front, top, PL, stream);
        else if (epw == 2) launch_obs_planes<1, 2>(P, front, top, PL, stream);
        else launch_obs_planes<1, 1>(P, front, top, PL, stream);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int lcr_launch_render_bg_planes(const LcrDev &P, const LcrCam &front, const LcrCam &top, const LcrPlanes &PL, void *stream) {
    hipLaunchKernelGGL(lcr_render_bg_planes_kernel, dim3((2 * P.img_w * P.img_h + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, front, top, PL);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int lcr_launch_render_single_planes(const LcrDev &P, const LcrCam &cam, int env, int W, int H, float far, float *depth_dev, unsigned char *seg_dev, void *stream) {
    hipLaunchKernelGGL(lcr_render_single_planes_kernel, dim3((W * H + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, cam, env, W, H, far, depth_dev, seg_dev);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
#endif

#if LCR_RENDER_LOOK
namespace {
template <int NV, int EPW>
void launch_obs_look(const LcrDev &P, const LcrLook &LK, const LcrPlanes *PL, void *stream) {
    const LcrCam none{};   // (the cameras come from the variants)
    const dim3 grid((P.n + EPW - 1) / EPW);
    if (PL) hipLaunchKernelGGL((lcr_render_obs_kernel<false, NV, EPW, 0, 0, LcrLook, LcrPlanes>), grid, dim3(256), (size_t)4 * 16 * P.img_w, (hipStream_t)stream, P, none, none, LK, *PL);
    else hipLaunchKernelGGL((lcr_render_obs_kernel<false, NV, EPW, 0, 0, LcrLook>), grid, dim3(256), (size_t)4 * 12 * P.img_w, (hipStream_t)stream, P, none, none, LK);
}
}  // namespace

// colour frames (+ the enabled planes when PL is given) with a look: the run-time-size builds at every size, same mappings as launch_obs_sized
int lcr_launch_render_obs_look(const LcrDev &P, const LcrLook &LK, const LcrPlanes *PL, void *stream) {
    if (!P.img_front || !P.img_top || !LK.var || !LK.bg || !LK.variant || !LK.rgb || (PL && (!PL->bg_depth || !PL->bg_seg))) return (int)hipErrorInvalidValue;
    const int nv = (3 * P.img_w / 4 + 63) / 64, epw = P.img_epw;
    if (nv > 4) launch_obs_look<6, 1>(P, LK, PL, stream);
    else if (nv > 2) launch_obs_look<4, 1>(P, LK, PL, stream);
    else if (nv > 1) {
        if (epw == 4) launch_obs_look<2, 4>(P, LK, PL, stream);
        else if (epw == 2) launch_obs_look<2, 2>(P, LK, PL, stream);
        else launch_obs_look<2, 1>(P, LK, PL, stream);
    } else {
        if (epw == 4) launch_obs_look<1, 4>(P, LK, PL, stream);
        else if (epw == 2) launch_obs_look<1, 2>(P, LK, PL, stream);
        else launch_obs_look<1, 1>(P, LK, PL, stream);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int lcr_launch_render_bg_look(const LcrDev &P, const LcrLook &LK, int K, void *stream) {
    hipLaunchKernelGGL(lcr_render_bg_look_kernel, dim3((K * 2 * P.img_w * P.img_h + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, LK, K);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int lcr_launch_render_bg_planes_look(const LcrDev &P, const LcrLook &LK, int K, const LcrPlanes &PL, void *stream) {
    hipLaunchKernelGGL(lcr_render_bg_planes_look_kernel, dim3((K * 2 * P.img_w * P.img_h + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, LK, K, PL);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int lcr_launch_render_single_look(const LcrDev &P, const LcrCam &cam, int env, int W, int H, unsigned char *out_dev, const LcrLook &LK, int look_env, int look_n, void *stream) {
    hipLaunchKernelGGL(lcr_render_single_look_kernel, dim3((W * H + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, cam, env, W, H, out_dev, LK, look_env, look_n);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int lcr_launch_look_redraw(int n, long long env_off, const unsigned char *flag, int mode, const LcrLookSampler &SM, int *cur, unsigned *episode, int *term, void *stream) {
    hipLaunchKernelGGL(lcr_look_redraw_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, env_off, flag, mode, SM, cur, episode, term);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int lcr_launch_look_gather(const int *ids_dev, int count, int n, const int *look, int *out, void *stream) {
    hipLaunchKernelGGL(lcr_look_gather_kernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, ids_dev, count, n, look, out);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
#endif

#if LCR_RENDER_SMALL
int lcr_launch_gather_terminal(const LcrDev &P, const int *ids_dev, int count, float *qpos_out, float *target_out, void *stream) {
    hipLaunchKernelGGL(lcr_gather_terminal_kernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, ids_dev, count, qpos_out, target_out);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

// Envs per workgroup of the frame kernel, from the frame size alone (profiles/frame_sizes.txt: four envs per workgroup take 0.461 instead of 0.499 ms at
// 64 x 64 and 0.587 instead of 0.624 at 84 x 84, 32 768 envs; at 128 x 128 the mappings measure the same, 0.97-0.98 ms; larger frames were not measured and keep one)
int lcr_render_envs_per_workgroup(int W, int H) {
    if (W > 170) return 1;   // (the several-envs builds exist for NV <= 2 only)
    return W * H <= 128 * 128 ? 4 : 1;
}

int lcr_launch_render_obs(const LcrDev &P, const LcrCam &front, const LcrCam &top, void *stream) {
    if (!P.img_front || !P.img_top) return 0;
    static const int count = [] { const char *e = getenv("LCR_RENDER_COUNT"); return e ? atoi(e) : 0; }();   // diagnostics: tools/render_work.py
    if (P.img_w != 320 || P.img_h != 240) lcr_launch_render_obs_sized(P, front, top, count != 0, stream);
    else if (count) launch_obs<true, 4, 1, 320, 240>(P, front, top, stream);
    else launch_obs<false, 4, 1, 320, 240>(P, front, top, stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int lcr_launch_render_bg(const LcrDev &P, const LcrCam &front, const LcrCam &top, void *stream) {
    if (!P.img_bg) return 0;
    hipLaunchKernelGGL(lcr_render_bg_kernel, dim3((2 * P.img_w * P.img_h + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, front, top);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int lcr_launch_render_single(const LcrDev &P, const LcrCam &cam, int env, int W, int H, unsigned char *out_dev, void *stream) {
    hipLaunchKernelGGL(lcr_render_single_kernel, dim3((W * H + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, cam, env, W, H, out_dev);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
#endif

#if LCR_RENDER_WRIST
namespace {
template <bool PLANES, bool LOOK>
void launch_wrist(const LcrDev &P, const LcrWrist &WR, const LcrLook &LK, void *stream) {
    const int epw = P.img_epw;
    const size_t lds = (size_t)4 * (PLANES ? 16 : 12) * P.img_w;
    if (epw == 4) hipLaunchKernelGGL((lcr_render_wrist_kernel<PLANES, LOOK, 4>), dim3((P.n + 3) / 4), dim3(256), lds, (hipStream_t)stream, P, WR, LK);
    else if (epw == 2) hipLaunchKernelGGL((lcr_render_wrist_kernel<PLANES, LOOK, 2>), dim3((P.n + 1) / 2), dim3(256), lds, (hipStream_t)stream, P, WR, LK);
    else hipLaunchKernelGGL((lcr_render_wrist_kernel<PLANES, LOOK, 1>), dim3(P.n), dim3(256), lds, (hipStream_t)stream, P, WR, LK);
}
}  // namespace

// the batched wrist frames (+ the planes WR points at; LK: with the envs' looks): the mapping by frame size of the two-camera frame kernel (P.img_epw)
int lcr_launch_render_wrist(const LcrDev &P, const LcrWrist &WR, const LcrLook *LK, void *stream) {
    if (!WR.img || (LK && (!LK->var || !LK->variant || !LK->rgb))) return (int)hipErrorInvalidValue;
    const bool planes = WR.depth || WR.seg;
    const LcrLook none{};
    if (LK) { if (planes) launch_wrist<true, true>(P, WR, *LK, stream); else launch_wrist<false, true>(P, WR, *LK, stream); }
    else { if (planes) launch_wrist<true, false>(P, WR, none, stream); else launch_wrist<false, false>(P, WR, none, stream); }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int lcr_launch_render_single_wrist(const LcrDev &P, const LcrWristMount &M, int env, int W, int H, float far, unsigned char *rgb_dev, float *depth_dev, unsigned char *seg_dev,
                                   const LcrLook *LK, int look_env, int look_n, void *stream) {
    const LcrLook none{};
    hipLaunchKernelGGL(lcr_render_single_wrist_kernel, dim3((W * H + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, M, env, W, H, far, rgb_dev, depth_dev, seg_dev,
                       LK ? *LK : none, LK ? look_env : -1, look_n);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
#endif
