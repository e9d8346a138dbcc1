// raster_pre_body.h -- per-Gaussian bodies of the preprocess forward / backward kernels, written as
// host+device functions over plain pointers so that tests/hostcheck can run exactly this code on the CPU.
#pragma once
#include "../../include/d3ga.h"
#include "d3ga_math.h"

namespace d3ga {

D3GA_HD V3 ld3(const float *p, size_t i) { return v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }

struct PreOut {
    Splat sp;
    float c6[6];
    float rgb[3];
    float opacity;
    uint8_t clampmask;
};

// The unit view direction of a Gaussian: normalize(mean - campos), as in R1.  Without contraction, like sh_basis: the
// inference forward and the forward that also leaves d(colour)/d(direction) must evaluate the same basis values.
// By value: the kernels load the mean once and hand it to the direction and to the projection; the pointer forms load it.
D3GA_HD void sh_view_dir(V3 m, const float *campos, float &x, float &y, float &z) {
    D3GA_NO_CONTRACT
    const float dx = m.x - campos[0], dy = m.y - campos[1], dz = m.z - campos[2];
    const float inv = 1.0f / sqrtf(dx * dx + dy * dy + dz * dz);
    x = dx * inv; y = dy * inv; z = dz * inv;
}
D3GA_HD void sh_view_dir(const float *means3D, int i, const float *campos, float &x, float &y, float &z) {
    sh_view_dir(ld3(means3D, i), campos, x, y, z);
}
// SH basis of a Gaussian's view direction
D3GA_HD void sh_view_basis(const d3ga_raster_params &prm, V3 m, const float *campos, float B[16]) {
    float x, y, z;
    sh_view_dir(m, campos, x, y, z);
    sh_basis(prm.sh_degree, x, y, z, B);
}
D3GA_HD void sh_view_basis(const d3ga_raster_params &prm, const float *means3D, int i, const float *campos, float B[16]) {
    sh_view_basis(prm, ld3(means3D, i), campos, B);
}
// acc[c] += sum_k B[k] * coeff[k][c]  AND  J[3 dir + c] = sum_k dY_k/d(dir)(x, y, z) * coeff[k][c] -- the derivative of the
// (unclamped, un-offset) SH colour w.r.t. the unit direction -- in ONE walk over the row: every coefficient is read once and
// the three derivative values of a basis function are formed where they are used (no 3 x 16 gradient arrays: the forward's
// staging kernel has no registers for them).  Same polynomials as sh_basis_grad.  Without contraction, the sums by explicit fmaf:
// the function is inlined into the forward's full-wavefront path and into its generic slab path, and the compiler contracted the
// two copies differently -- J, and with it dL/dmeans3D of the same Gaussian, then depended in the last bit on whether its row
// fell into a full wavefront (tests/test_gpu_preprocess_alone.py: layout).
struct ShColJ { float a0, a1, a2, j0, j1, j2, j3, j4, j5, j6, j7, j8; };      // by value: as arrays behind pointers these landed in scratch memory
D3GA_HD ShColJ sh_accumulate_jacobian(const float B[16], float x, float y, float z, const float *row, int nb, ShColJ o) {
    D3GA_NO_CONTRACT
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    o.j0 = o.j1 = o.j2 = o.j3 = o.j4 = o.j5 = o.j6 = o.j7 = o.j8 = 0.f;
#define D3GA_SHJ(K, GX, GY, GZ)                                                                             \
    if (K < nb) {                                                                                           \
        const float r0 = row[3 * K], r1 = row[3 * K + 1], r2 = row[3 * K + 2];                              \
        o.a0 = fmaf(B[K], r0, o.a0); o.a1 = fmaf(B[K], r1, o.a1); o.a2 = fmaf(B[K], r2, o.a2);   /* as sh_accumulate, bit for bit */                                            \
        const float gx_ = (GX), gy_ = (GY), gz_ = (GZ);                                                     \
        o.j0 = fmaf(gx_, r0, o.j0); o.j1 = fmaf(gx_, r1, o.j1); o.j2 = fmaf(gx_, r2, o.j2);                 \
        o.j3 = fmaf(gy_, r0, o.j3); o.j4 = fmaf(gy_, r1, o.j4); o.j5 = fmaf(gy_, r2, o.j5);                 \
        o.j6 = fmaf(gz_, r0, o.j6); o.j7 = fmaf(gz_, r1, o.j7); o.j8 = fmaf(gz_, r2, o.j8);                 \
    }
    if (0 < nb) { o.a0 = fmaf(B[0], row[0], o.a0); o.a1 = fmaf(B[0], row[1], o.a1); o.a2 = fmaf(B[0], row[2], o.a2); }
    D3GA_SHJ(1, 0.f, -kC1, 0.f)
    D3GA_SHJ(2, 0.f, 0.f, kC1)
    D3GA_SHJ(3, -kC1, 0.f, 0.f)
    D3GA_SHJ(4, kC2_0 * y, kC2_0 * x, 0.f)
    D3GA_SHJ(5, 0.f, kC2_1 * z, kC2_1 * y)
    D3GA_SHJ(6, -2.f * kC2_2 * x, -2.f * kC2_2 * y, 4.f * kC2_2 * z)
    D3GA_SHJ(7, kC2_3 * z, 0.f, kC2_3 * x)
    D3GA_SHJ(8, 2.f * kC2_4 * x, -2.f * kC2_4 * y, 0.f)
    D3GA_SHJ(9, kC3_0 * 6.f * xy, kC3_0 * 3.f * (xx - yy), 0.f)
    D3GA_SHJ(10, kC3_1 * yz, kC3_1 * xz, kC3_1 * xy)
    D3GA_SHJ(11, kC3_2 * -2.f * xy, kC3_2 * (4.f * zz - xx - 3.f * yy), kC3_2 * 8.f * yz)
    D3GA_SHJ(12, kC3_3 * -6.f * xz, kC3_3 * -6.f * yz, kC3_3 * 3.f * (2.f * zz - xx - yy))
    D3GA_SHJ(13, kC3_4 * (4.f * zz - 3.f * xx - yy), kC3_4 * -2.f * xy, kC3_4 * 8.f * xz)
    D3GA_SHJ(14, kC3_5 * 2.f * xz, kC3_5 * -2.f * yz, kC3_5 * (xx - yy))
    D3GA_SHJ(15, kC3_6 * 3.f * (xx - yy), kC3_6 * -6.f * xy, 0.f)
#undef D3GA_SHJ
    return o;
}
// acc[c] += sum_{k in [k0, k1)} B[k] * coeff[k][c];  `part` points at coefficient k0 of the row (3 floats per coefficient)
D3GA_HD void sh_accumulate(const float B[16], const float *part, int k0, int k1, int nb, float acc[3]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {           // fixed trip count: keeps B[] in registers
        if (k >= k0 && k < k1 && k < nb) {
            const float *c = part + 3 * (k - k0);
            acc[0] = fmaf(B[k], c[0], acc[0]); acc[1] = fmaf(B[k], c[1], acc[1]); acc[2] = fmaf(B[k], c[2], acc[2]);   // explicit: the same in every caller
        }
    }
}

// One view's camera.  The only code that reads the camera-slot convention (d3ga.h): tanfovx <= 0 puts the two tangents behind
// the position (campos[3], campos[4]); a WINDOWED slot (9 floats) adds the full raster's size (campos[5], campos[6]), which the
// view projects with, and the window's origin in it (campos[7], campos[8]).
struct ViewCam {
    const float *vm, *pm, *cp;      // view matrix, projection matrix, camera row
    float tanfovx, tanfovy;
    int W, H;                       // the raster the view projects on
    int ox, oy;                     // (windowed) the window's first pixel in that raster
};
D3GA_HD ViewCam view_cam(const d3ga_raster_params &prm, const float *vm, const float *pm, const float *cp, bool win) {
    ViewCam c = {vm, pm, cp, prm.tanfovx, prm.tanfovy, prm.W, prm.H, 0, 0};
    if (!(prm.tanfovx > 0.f)) { c.tanfovx = cp[3]; c.tanfovy = cp[4]; }
    if (win) { c.W = (int)cp[5]; c.H = (int)cp[6]; c.ox = (int)cp[7]; c.oy = (int)cp[8]; }
    return c;
}
// the cameras of up to K views of a batch, by value (kernel arguments)
template <int K>
struct ViewCams { const float *vm[K], *pm[K], *cp[K]; };

// Records the preprocess forward leaves and the compositing backward accumulates (d3ga_internal.h: GeomBuf; d3ga.h: acc),
// as plain pointers.  A culled Gaussian keeps an EMPTY tile rectangle (x = minx | miny << 16, y = maxx | maxy << 16).
D3GA_HD bool rect_visible(uint32_t lo, uint32_t hi) { return ((hi & 0xffffu) > (lo & 0xffffu)) && ((hi >> 16) > (lo >> 16)); }
// accumulator record j (D3GA_ACC_STRIDE floats, 64-byte aligned).  self_clearing (d3ga_raster_params::acc_self_clearing): the
// caller keeps the buffer for the next backward -- leave the record as the untouched ones are, all zero (only records the
// compositing backward wrote are written back: 48 of their 64 bytes)
struct AccRec { float a[12]; };
D3GA_HD AccRec acc_load(const float *acc, size_t j, bool self_clearing) {
    float *p = (float *)__builtin_assume_aligned(const_cast<float *>(acc) + D3GA_ACC_STRIDE * j, 64);
    AccRec r;
    uint32_t any = 0;
    for (int k = 0; k < 12; ++k) { r.a[k] = p[k]; any |= __builtin_bit_cast(uint32_t, r.a[k]); }
    if (self_clearing && any)
        for (int k = 0; k < 12; ++k) p[k] = 0.f;
    return r;
}
// d(SH colour)/d(unit view direction) of record j: nine planes of `stride` floats (GeomBuf::dcol)
D3GA_HD ShColJ dcol_load(const float *dcol, int64_t stride, size_t j) {
    ShColJ c = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    c.j0 = dcol[j]; c.j1 = dcol[stride + j]; c.j2 = dcol[2 * stride + j];
    c.j3 = dcol[3 * stride + j]; c.j4 = dcol[4 * stride + j]; c.j5 = dcol[5 * stride + j];
    c.j6 = dcol[6 * stride + j]; c.j7 = dcol[7 * stride + j]; c.j8 = dcol[8 * stride + j];
    return c;
}
D3GA_HD void dcol_store(float *dcol, int64_t stride, size_t j, const ShColJ &c) {
    dcol[j] = c.j0; dcol[stride + j] = c.j1; dcol[2 * stride + j] = c.j2;
    dcol[3 * stride + j] = c.j3; dcol[4 * stride + j] = c.j4; dcol[5 * stride + j] = c.j5;
    dcol[6 * stride + j] = c.j6; dcol[7 * stride + j] = c.j7; dcol[8 * stride + j] = c.j8;
}

// R1 for Gaussian i in the view `cam`.  Exactly one of (sh_row|sh_acc|colors_precomp), ((scales,rotations)|cov3D_precomp) is non-null.
// sh_row points at THIS Gaussian's 3*M SH floats (in global memory or in an LDS staging row); alternatively pl.sh
// holds the already evaluated sum_k Y_k(dir) * coeff_k (see sh_view_basis / sh_accumulate).
// pl.c6 / pl.op: this Gaussian's covariance row and raw opacity if the caller has loaded them already (the kernel issues
// those loads before it stages the SH rows).  The opacity is read unconditionally: behind the visibility test it would be
// one more dependent memory round trip per wavefront.
// What the caller has in registers already, BY VALUE (round 4: as nullable pointers to locals these lived in scratch
// memory -- 69 scratch instructions in the kernel and a dependent memory round trip in front of the colour).
struct PreLoaded {
    bool has_sh = false, has_c6 = false;   // uniform over the launch
    bool has_mean = false;                 // uniform over the launch: `mean` is means3D[i], loaded by the caller (once per Gaussian)
    float sh[3] = {0.f, 0.f, 0.f};         // sum_k Y_k(dir) * coeff_k, already evaluated (sh_view_basis / sh_accumulate)
    float c6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float op = 0.f;                        // raw opacity (with has_c6)
    V3 mean = {0.f, 0.f, 0.f};
};
// R1 in two steps, so that a kernel can run the projection (and what hangs on the tile rectangle) while the SH rows are still
// in flight: preprocess_geom is everything that needs mean, covariance, opacity and camera only; preprocess_colour fills in
// rgb / clampmask of a visible Gaussian.  preprocess_one is the two in a row.
D3GA_HD PreOut preprocess_geom(const d3ga_raster_params &prm, const ViewCam &cam, int i, V3 mean, const float *opacities,
                               const float *scales, const float *rotations, const float *cov3D_precomp, const PreLoaded &pl) {
    PreOut o;
    const float raw_opacity = pl.has_c6 ? pl.op : opacities[i];
    if (pl.has_c6) {
        for (int k = 0; k < 6; ++k) o.c6[k] = pl.c6[k];
    } else if (cov3D_precomp) {
        for (int k = 0; k < 6; ++k) o.c6[k] = cov3D_precomp[6 * (size_t)i + k];
    } else {
        const float s[3] = {scales[3 * (size_t)i], scales[3 * (size_t)i + 1], scales[3 * (size_t)i + 2]};
        const float q[4] = {rotations[4 * (size_t)i], rotations[4 * (size_t)i + 1], rotations[4 * (size_t)i + 2],
                            rotations[4 * (size_t)i + 3]};
        cov3d_from_scale_rot(s, prm.scale_modifier, q, o.c6);
    }
    o.sp = project_gaussian(mean, o.c6, cam.vm, cam.pm, cam.W, cam.H, cam.tanfovx, cam.tanfovy, prm.antialiasing != 0);
    o.rgb[0] = o.rgb[1] = o.rgb[2] = 0.f;
    o.clampmask = 0;
    o.opacity = 0.f;
    if (!o.sp.visible) return o;
    o.opacity = raw_opacity;
    if (prm.opacity_activation == D3GA_OPACITY_SIGMOID) o.opacity = 1.0f / (1.0f + expf(-o.opacity));   // cage_net.py:247
    if (!(o.opacity == o.opacity)) {         // NaN opacity: min(0.99, NaN * G) would evaluate to 0.99 -- cull instead
        o.sp.visible = false; o.sp.radius = 0;
        o.sp.rect[0] = o.sp.rect[1] = o.sp.rect[2] = o.sp.rect[3] = 0;
        o.opacity = 0.f;
        return o;
    }
    o.opacity *= o.sp.aa;                    // antialiasing (branch dr_aa): what the compositing stage sees is opacity x h_convolution_scaling
    return o;
}
// visible: o.sp.visible as preprocess_geom left it (a window clip behind it does not count)
D3GA_HD void preprocess_colour(const d3ga_raster_params &prm, const ViewCam &cam, int i, V3 mean, const float *sh_row,
                               const float *colors_precomp, const PreLoaded &pl, bool visible, float (&rgb)[3], uint8_t &clampmask) {
    if (!visible) return;
    if (colors_precomp) {
        rgb[0] = colors_precomp[3 * (size_t)i]; rgb[1] = colors_precomp[3 * (size_t)i + 1];
        rgb[2] = colors_precomp[3 * (size_t)i + 2];
    } else {
        float acc[3] = {0.f, 0.f, 0.f};
        if (pl.has_sh) {
            acc[0] = pl.sh[0]; acc[1] = pl.sh[1]; acc[2] = pl.sh[2];
        } else {
            float B[16];
            sh_view_basis(prm, mean, cam.cp, B);
            sh_accumulate(B, sh_row, 0, 16, (prm.sh_degree + 1) * (prm.sh_degree + 1), acc);
        }
        for (int c = 0; c < 3; ++c) {
            const float v = acc[c] + 0.5f;
            if (v < 0.f) clampmask |= (uint8_t)(1u << c);
            rgb[c] = fmaxf(v, 0.f);
        }
    }
}
D3GA_HD PreOut preprocess_one(const d3ga_raster_params &prm, const ViewCam &cam, int i, const float *means3D, const float *sh_row,
                              const float *colors_precomp, const float *opacities, const float *scales,
                              const float *rotations, const float *cov3D_precomp, const PreLoaded pl = PreLoaded()) {
    const V3 mean = pl.has_mean ? pl.mean : ld3(means3D, i);
    PreOut o = preprocess_geom(prm, cam, i, mean, opacities, scales, rotations, cov3D_precomp, pl);
    preprocess_colour(prm, cam, i, mean, sh_row, colors_precomp, pl, o.sp.visible, o.rgb, o.clampmask);
    return o;
}

// The same with the camera as the params give it (tangents and raster size already those of this view: the host check).
D3GA_HD PreOut preprocess_one(const d3ga_raster_params &prm, int i, const float *means3D, const float *sh_row,
                              const float *colors_precomp, const float *opacities, const float *scales,
                              const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                              const float *projmatrix, const float *campos, const PreLoaded pl = PreLoaded()) {
    const ViewCam cam = {viewmatrix, projmatrix, campos, prm.tanfovx, prm.tanfovy, prm.W, prm.H, 0, 0};
    return preprocess_one(prm, cam, i, means3D, sh_row, colors_precomp, opacities, scales, rotations, cov3D_precomp, pl);
}

// R6 of ONE Gaussian in ONE view: the gradients its screen-space accumulator record a[12] (layout: d3ga.h,
// d3ga_raster_composite_bwd) sends to its mean and covariance, to its opacity (gop) and -- SH colours (sh) -- the clamp-masked
// dL/dcolour gr and the view direction's SH basis B (the view's SH gradient row is B (x) gr).  Zero for a culled Gaussian, but
// for gop.  The direction term of the mean's gradient comes from the forward's d(colour)/d(direction) jd (have_j) or from the
// coefficient row sh_row.  c6: the covariance the forward projected; act_opacity: the opacity it stored (conic_o.w).
// dsh_row (may be null, may alias sh_row): the view's SH gradient row B (x) gr is also written there, in the same walk over the
// coefficients -- with the row written after the walk, the compiler hoists all 48 coefficient loads and the single-view
// backward needs 22 more VGPRs (one occupancy step).
struct BwdView { float gmean[3], g6[6], gr[3], B[16], gop; };
D3GA_HD BwdView preprocess_bwd_view(const d3ga_raster_params &prm, const ViewCam &cam, bool visible, V3 mean, const float *c6,
                                    const float *a, uint8_t clampmask, float act_opacity, bool sh, bool have_j, ShColJ jd,
                                    const float *sh_row, float *dsh_row = nullptr) {
    BwdView r;       // (the sums below in local arrays: accumulated in the struct, the single-view backward needs 12 more VGPRs)
    float gmean[3] = {0.f, 0.f, 0.f}, g6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    r.gr[0] = r.gr[1] = r.gr[2] = 0.f;
    float aa = 1.0f;
    if (visible) {
        cov2d_bwd(mean, c6, cam.vm, cam.W, cam.H, cam.tanfovx, cam.tanfovy, a[3], a[4], a[5], g6, gmean,
                  prm.antialiasing != 0, a[6], act_opacity, &aa);
        project_bwd(mean, cam.pm, a[0], a[1], gmean);
        // inverse depth (branch dr_aa): a[10] = dL/d(1/z) of this Gaussian, z its view-space depth; d(1/z)/dmean = -view_z / z^2
        const float *vm = cam.vm;
        const float z = vm[2] * mean.x + vm[6] * mean.y + vm[10] * mean.z + vm[14];
        const float gz = -a[10] / (z * z);
        gmean[0] += vm[2] * gz; gmean[1] += vm[6] * gz; gmean[2] += vm[10] * gz;
    }
    if (sh && visible) {
        r.gr[0] = (clampmask & 1) ? 0.f : a[7]; r.gr[1] = (clampmask & 2) ? 0.f : a[8]; r.gr[2] = (clampmask & 4) ? 0.f : a[9];
        const float *gr = r.gr;
        float B[16];
        const V3 d0 = mean - v3(cam.cp[0], cam.cp[1], cam.cp[2]);
        const float inv = 1.0f / sqrtf(dot(d0, d0));
        const float x = d0.x * inv, y = d0.y * inv, z = d0.z * inv;
        sh_basis(prm.sh_degree, x, y, z, B);
        const int nb = (prm.sh_degree + 1) * (prm.sh_degree + 1), nbM = prm.M;
        float *out = dsh_row;
        V3 gd = v3(0.f, 0.f, 0.f);
        if (have_j) {                        // dL/d(dir) = J . (clamp-masked dL/dcolour): the coefficients are not read
            gd = v3(jd.j0 * gr[0] + jd.j1 * gr[1] + jd.j2 * gr[2], jd.j3 * gr[0] + jd.j4 * gr[1] + jd.j5 * gr[2],
                    jd.j6 * gr[0] + jd.j7 * gr[1] + jd.j8 * gr[2]);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (k < nb) { if (out) { out[3 * k] = B[k] * gr[0]; out[3 * k + 1] = B[k] * gr[1]; out[3 * k + 2] = B[k] * gr[2]; } }
                else if (k < nbM && out) { out[3 * k] = 0.f; out[3 * k + 1] = 0.f; out[3 * k + 2] = 0.f; }
            }
        } else {
            float Bx[16], By[16], Bz[16];
            sh_basis_grad(prm.sh_degree, x, y, z, Bx, By, Bz);
            const float *sh = sh_row;
#pragma unroll
            for (int k = 0; k < 16; ++k) {   // fixed trip count: keeps the basis arrays in registers
                if (k < nb) {
                    const float s0 = sh[3 * k], s1 = sh[3 * k + 1], s2 = sh[3 * k + 2];
                    if (out) { out[3 * k] = B[k] * gr[0]; out[3 * k + 1] = B[k] * gr[1]; out[3 * k + 2] = B[k] * gr[2]; }
                    const float w = s0 * gr[0] + s1 * gr[1] + s2 * gr[2];
                    gd.x += Bx[k] * w; gd.y += By[k] * w; gd.z += Bz[k] * w;
                } else if (k < nbM && out) {
                    out[3 * k] = 0.f; out[3 * k + 1] = 0.f; out[3 * k + 2] = 0.f;
                }
            }
        }
        const V3 gm = normalize_bwd(d0, gd);
        gmean[0] += gm.x; gmean[1] += gm.y; gmean[2] += gm.z;
        for (int k = 0; k < 16; ++k) r.B[k] = B[k];
    }
    // sigmoid' = s (1 - s); antialiasing: the stored opacity is opacity x aa and a[6] is the gradient w.r.t. that product
    const float op = act_opacity / aa, g_op = a[6] * aa;
    for (int k = 0; k < 3; ++k) r.gmean[k] = gmean[k];
    for (int k = 0; k < 6; ++k) r.g6[k] = g6[k];
    r.gop = prm.opacity_activation == D3GA_OPACITY_SIGMOID ? g_op * op * (1.0f - op) : g_op;
    return r;
}

// R6 for Gaussian i in one view.  a[12] = its accumulator record; all-zero and visible=false for culled Gaussians.  Output
// pointers may be null where not applicable.  sh_row / dsh_row point at THIS Gaussian's 3*M floats (global memory or an LDS
// staging row; they may alias).  have_j: jd = the forward's d(colour)/d(direction) of this Gaussian (then sh_row is not read).
// accum: views > 0 of a batch (d3ga.h n_views): gradients of inputs the views SHARE are added to what the outputs hold -- bit 0:
// opacity and a precomputed colour, bit 1: the geometry (mean, covariance | scale, rotation).
D3GA_HD void preprocess_bwd_one(const d3ga_raster_params &prm, const ViewCam &cam, int i, bool visible, const float *means3D,
                                const float *sh_row, const float *scales, const float *rotations,
                                const float *c6, uint8_t clampmask, const float *a, float *dL_dmeans3D,
                                float *dL_dmeans2D, float *dL_dopacity, float *dsh_row, float *dL_dcolors,
                                float *dL_dcov3D, float *dL_dscales, float *dL_drots, float act_opacity = 0.f,
                                bool have_j = false, ShColJ jd = ShColJ(), int accum = 0) {
    // SH colour path (sh_row != null).  dsh_row == null selects the FACTORED output used by the view-sharded gradient
    // exchange (d3ga_sh_grad_from_views): the clamp-masked dL/dcolour is written to dL_dcolors instead of the rank-1
    // (basis x dL/dcolour) SH block; the view-direction term of dL/dmean is computed either way.
    const BwdView r = preprocess_bwd_view(prm, cam, visible, ld3(means3D, i), c6, a, clampmask, act_opacity, sh_row != nullptr,
                                          have_j, jd, sh_row, dsh_row);
    if (sh_row) {
        float *out = dsh_row;
        if (visible) {
            if (dL_dcolors) {
                dL_dcolors[3 * (size_t)i] = r.gr[0]; dL_dcolors[3 * (size_t)i + 1] = r.gr[1]; dL_dcolors[3 * (size_t)i + 2] = r.gr[2];
            }
        } else {
            if (out) for (int k = 0; k < 3 * prm.M; ++k) out[k] = 0.f;
            if (dL_dcolors) {
                dL_dcolors[3 * (size_t)i] = 0.f; dL_dcolors[3 * (size_t)i + 1] = 0.f; dL_dcolors[3 * (size_t)i + 2] = 0.f;
            }
        }
    } else if (dL_dcolors) {                 // a precomputed colour is view-independent: summed over a batch's views
        float *o = dL_dcolors + 3 * (size_t)i;
        o[0] = (accum & 1) ? o[0] + (a[7]) : (a[7]); o[1] = (accum & 1) ? o[1] + (a[8]) : (a[8]); o[2] = (accum & 1) ? o[2] + (a[9]) : (a[9]);
    }
    {
        float *o = dL_dmeans3D + 3 * (size_t)i;
        o[0] = (accum & 2) ? o[0] + (r.gmean[0]) : (r.gmean[0]); o[1] = (accum & 2) ? o[1] + (r.gmean[1]) : (r.gmean[1]); o[2] = (accum & 2) ? o[2] + (r.gmean[2]) : (r.gmean[2]);
    }
    if (dL_dmeans2D) {                       // screen-space: per view
        dL_dmeans2D[3 * (size_t)i] = a[0]; dL_dmeans2D[3 * (size_t)i + 1] = a[1]; dL_dmeans2D[3 * (size_t)i + 2] = 0.f;
    }
    if (dL_dopacity) dL_dopacity[i] = (accum & 1) ? dL_dopacity[i] + r.gop : r.gop;
    if (dL_dcov3D) {
        for (int k = 0; k < 6; ++k) dL_dcov3D[6 * (size_t)i + k] = (accum & 2) ? dL_dcov3D[6 * (size_t)i + k] + (r.g6[k]) : (r.g6[k]);
    }
    if (dL_dscales && dL_drots) {
        float gs[3] = {0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f};
        if (visible) {
            const float s[3] = {scales[3 * (size_t)i], scales[3 * (size_t)i + 1], scales[3 * (size_t)i + 2]};
            const float q[4] = {rotations[4 * (size_t)i], rotations[4 * (size_t)i + 1], rotations[4 * (size_t)i + 2],
                                rotations[4 * (size_t)i + 3]};
            cov3d_from_scale_rot_bwd(s, prm.scale_modifier, q, r.g6, gs, gq);
        }
        for (int k = 0; k < 3; ++k) dL_dscales[3 * (size_t)i + k] = (accum & 2) ? dL_dscales[3 * (size_t)i + k] + (gs[k]) : (gs[k]);
        for (int k = 0; k < 4; ++k) dL_drots[4 * (size_t)i + k] = (accum & 2) ? dL_drots[4 * (size_t)i + k] + (gq[k]) : (gq[k]);
    }
}

// The same with the camera as the params give it (see preprocess_one).
D3GA_HD void preprocess_bwd_one(const d3ga_raster_params &prm, int i, bool visible, const float *means3D,
                                const float *sh_row, const float *scales, const float *rotations,
                                const float *viewmatrix, const float *projmatrix, const float *campos,
                                const float *c6, uint8_t clampmask, const float *a, float *dL_dmeans3D,
                                float *dL_dmeans2D, float *dL_dopacity, float *dsh_row, float *dL_dcolors,
                                float *dL_dcov3D, float *dL_dscales, float *dL_drots, float act_opacity = 0.f,
                                bool have_j = false, ShColJ jd = ShColJ(), int accum = 0) {
    const ViewCam cam = {viewmatrix, projmatrix, campos, prm.tanfovx, prm.tanfovy, prm.W, prm.H, 0, 0};
    preprocess_bwd_one(prm, cam, i, visible, means3D, sh_row, scales, rotations, c6, clampmask, a, dL_dmeans3D, dL_dmeans2D,
                       dL_dopacity, dsh_row, dL_dcolors, dL_dcov3D, dL_dscales, dL_drots, act_opacity, have_j, jd, accum);
}

// The records a batch's backward reads per view (GeomBuf of the batch's first view, acc of that view): record j = v P + i.
struct ViewRecs {
    const uint32_t *rect;        // 2 words per record
    const float *acc;            // D3GA_ACC_STRIDE floats per record
    const uint8_t *clamped;
    const float *conic_o;        // 4 floats per record: the stored opacity is [3]
    const float *dcol;           // SH colours: the forward's d(colour)/d(direction), nine planes of dcol_stride floats
    int64_t dcol_stride;
};
// R6 of Gaussian i over the kv views of a batch that share their geometry (d3ga.h: n_views), in ONE walk: per view its records and
// preprocess_bwd_view, the gradients of the shared inputs summed in registers, views added in ascending order (so: the same sums as kv
// calls of preprocess_bwd_one with `accum`), every output written ONCE.  The SH gradient row, sum_v B_v (x) gr_v, goes to dsh_row
// (null: not wanted); SH colours need the forward's dcol.  cov6: the covariance rows the forward projected.  pv: records between
// the views' geometry AND geometry gradients -- 0: shared (summed), P: a batch of frames (written per view).  pva: per-view
// appearance -- dL/dopacity and dL/dcolour are written per view at record j (zeros where the view culled the Gaussian), not summed.
// accum: add to every output that is not per view (a later group of a large batch).
template <int K>
D3GA_HD void preprocess_bwd_views_one(const d3ga_raster_params &prm, int i, int kv, bool win, const ViewCams<K> &cams,
                                      const ViewRecs &rec, const float *means3D, const float *cov6, const float *scales,
                                      const float *rotations, bool sh_path, size_t pv, bool pva, bool accum,
                                      float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dopacity, float *dL_dcolors,
                                      float *dL_dcov3D, float *dL_dscales, float *dL_drots, float *dsh_row) {
    V3 mean = ld3(means3D, i);
    float c6[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) c6[k] = cov6[6 * (size_t)i + k];   // (from scale / rotation: view 0's record -- the same in every view of shared geometry)
    float gmean[3] = {0.f, 0.f, 0.f}, g6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gop = 0.f, gcol[3] = {0.f, 0.f, 0.f};
    auto put = [&](float *p, float v, bool add) { *p = add ? *p + v : v; };
    auto geometry_out = [&](size_t og, const float (&gm)[3], const float (&g)[6], bool vis, bool add) {     // og: record offset of the geometry gradients
        for (int k = 0; k < 3; ++k) put(dL_dmeans3D + 3 * (og + i) + k, gm[k], add);
        if (dL_dcov3D)
            for (int k = 0; k < 6; ++k) put(dL_dcov3D + 6 * (og + i) + k, g[k], add);
        if (dL_dscales && dL_drots) {
            float gs[3] = {0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f};
            if (vis) {
                const float sc[3] = {scales[3 * (og + i)], scales[3 * (og + i) + 1], scales[3 * (og + i) + 2]};
                const float q[4] = {rotations[4 * (og + i)], rotations[4 * (og + i) + 1], rotations[4 * (og + i) + 2], rotations[4 * (og + i) + 3]};
                cov3d_from_scale_rot_bwd(sc, prm.scale_modifier, q, g, gs, gq);      // (linear in g: a sum over views goes through once)
            }
            for (int k = 0; k < 3; ++k) put(dL_dscales + 3 * (og + i) + k, gs[k], add);
            for (int k = 0; k < 4; ++k) put(dL_drots + 4 * (og + i) + k, gq[k], add);
        }
    };
    const float zero3[3] = {0.f, 0.f, 0.f}, zero6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int nb = (prm.sh_degree + 1) * (prm.sh_degree + 1);
    float out[48];
#pragma unroll
    for (int k = 0; k < 48; ++k) out[k] = 0.f;
    for (int v = 0; v < kv; ++v) {
        const size_t j = (size_t)prm.P * v + i;                          // this view's record
        const uint32_t r0 = rec.rect[2 * j], r1 = rec.rect[2 * j + 1];
        const AccRec ar = acc_load(rec.acc, j, prm.acc_self_clearing);
        const float *a = ar.a;
        const bool visible = rect_visible(r0, r1);
        if (dL_dmeans2D) {                                                // screen-space: per view
            float *m2 = dL_dmeans2D + 3 * j;
            m2[0] = visible ? a[0] : 0.f; m2[1] = visible ? a[1] : 0.f; m2[2] = 0.f;
        }
        if (!visible) {
            if (pv) geometry_out(pv * v, zero3, zero6, false, false);      // a batch of frames: every view's geometry gradients are written
            if (pva) {                                                     // ... and per-view appearance every view's opacity / colour gradients
                if (dL_dopacity) dL_dopacity[j] = 0.f;
                if (dL_dcolors) { dL_dcolors[3 * j] = 0.f; dL_dcolors[3 * j + 1] = 0.f; dL_dcolors[3 * j + 2] = 0.f; }
            }
            continue;
        }
        if (pv) {                                                        // this view's own geometry
            mean = ld3(means3D + 3 * pv * v, i);
#pragma unroll
            for (int k = 0; k < 6; ++k) c6[k] = cov6[6 * (pv * v + i) + k];
        }
        const ViewCam cam = view_cam(prm, cams.vm[v], cams.pm[v], cams.cp[v], win);
        const BwdView r = preprocess_bwd_view(prm, cam, true, mean, c6, a, rec.clamped[j], rec.conic_o[4 * j + 3], sh_path, true,
                                              sh_path ? dcol_load(rec.dcol, rec.dcol_stride, j) : ShColJ(), nullptr);
        if (sh_path) {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < nb) { out[3 * k] += r.B[k] * r.gr[0]; out[3 * k + 1] += r.B[k] * r.gr[1]; out[3 * k + 2] += r.B[k] * r.gr[2]; }
        } else if (pva) {
            if (dL_dcolors) { dL_dcolors[3 * j] = a[7]; dL_dcolors[3 * j + 1] = a[8]; dL_dcolors[3 * j + 2] = a[9]; }
        } else {
            gcol[0] += a[7]; gcol[1] += a[8]; gcol[2] += a[9];
        }
        if (!pva) gop += r.gop;
        else if (dL_dopacity) dL_dopacity[j] = r.gop;
        if (pv) geometry_out(pv * v, r.gmean, r.g6, true, false);
        else {
            gmean[0] += r.gmean[0]; gmean[1] += r.gmean[1]; gmean[2] += r.gmean[2];
#pragma unroll
            for (int k = 0; k < 6; ++k) g6[k] += r.g6[k];
        }
    }
    if (!pv) geometry_out(0, gmean, g6, true, accum);
    if (dL_dopacity && !pva) put(dL_dopacity + i, gop, accum);
    if (!sh_path && !pva && dL_dcolors) { put(dL_dcolors + 3 * (size_t)i, gcol[0], accum); put(dL_dcolors + 3 * (size_t)i + 1, gcol[1], accum); put(dL_dcolors + 3 * (size_t)i + 2, gcol[2], accum); }
    if (sh_path && dsh_row) {
#pragma unroll
        for (int k = 0; k < 48; ++k)
            if (k < 3 * prm.M) dsh_row[k] = out[k];
    }
}

}  // namespace d3ga
