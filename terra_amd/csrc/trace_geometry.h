// trace_geometry.h -- rays against boxes and triangles (trace_device.h lists the layers): the camera sample, the slab tests in their
// four forms, the watertight test in its two forms and the Moeller-Trumbore test.
#pragma once
#include "trace_math.h"

// -----------------------------------------------------------------------------
// camera
// -----------------------------------------------------------------------------
// the sample's film position in [-1, 1]^2 (sx to the right, sy up)
TD void camera_film ( const DevRenderParams& p, uint32_t px, uint32_t py, float r1, float r2, float& sx, float& sy ) {
    float dx = -p.jitter + 2 * r1 * p.jitter;
    float dy = -p.jitter + 2 * r2 * p.jitter;
    // x / fb_w, y / fb_h bit for bit: the reciprocals of the frame size are launch constants, rounded on the host (fill_camera), and 1 <= fb_w, fb_h <= 2^32 is inside
    // the range div_exact_rk asks of its caller
    float ndc_x, ndc_y; div2_exact_rk ( ( float ) px + 0.5f + dx, ( float ) py + 0.5f + dy, ( float ) p.fb_w, p.inv_fb_w, ( float ) p.fb_h, p.inv_fb_h, ndc_x, ndc_y );
    sx = 2 * ndc_x - 1;
    sy = 1 - 2 * ndc_y;
}
// world direction of a camera-space vector
TD V3 camera_rotate ( const DevRenderParams& p, V3 d ) {
    return v3 ( p.cam_rot[0] * d.x + p.cam_rot[1] * d.y + p.cam_rot[2] * d.z,
                p.cam_rot[3] * d.x + p.cam_rot[4] * d.y + p.cam_rot[5] * d.z,
                p.cam_rot[6] * d.x + p.cam_rot[7] * d.y + p.cam_rot[8] * d.z );
}
TD V3 camera_sample ( const DevRenderParams& p, uint32_t px, uint32_t py, float r1, float r2 ) {
    float sx, sy; camera_film ( p, px, py, r1, r2, sx, sy );
    float fx = sx * p.aspect * p.tan_half_fov;
    float fy = sy * p.tan_half_fov;
    V3 d = normalize ( v3 ( fx, fy, 1.f ) );
    return camera_rotate ( p, d );
}

// camera_sample for the kernels that shade in stages, in a launch whose constants passed terra_camera_stage_limits (dev_types.h: the bounds used here): the film
// vector's normalisation without a range test. Its squared length is in [1, 2^41], inside the short root's range; its length in [1, 2^21] and its components 0
// or above 2^-60, inside xd_normalize3's; a length whose significand is all ones takes the closed-form reciprocal (exact_div.h xd_rcp_all_ones). The film
// quotients keep their test (with jitter 0.5 the numerator at px = 0 can be exactly 0). Same bits as camera_sample: the unit entry's stage 5 holds
// camera_film_normalize to normalize_plain.
TD V3 camera_film_normalize ( float fx, float fy ) {
    const float l = xs_sqrt_short ( fx * fx + fy * fy + 1.f * 1.f ), r = xd_rcp_short_any ( l );
    return v3 ( xd_div_short_pos ( fx, l, r ), xd_div_short_pos ( fy, l, r ), xd_div_short_pos ( 1.f, l, r ) );
}
TD V3 camera_sample_staged ( const DevRenderParams& p, uint32_t px, uint32_t py, float r1, float r2 ) {
    if ( p.shade_s1_guarded || TERRA_SHADE_DROPS == 0 ) return camera_sample ( p, px, py, r1, r2 );          // (a launch constant: the branch is uniform)
    float sx, sy; camera_film ( p, px, py, r1, r2, sx, sy );
    return camera_rotate ( p, camera_film_normalize ( sx * p.aspect * p.tan_half_fov, sy * p.tan_half_fov ) );
}

// concentric map of a pair of draws to the unit disk (include/terra_amd.h "Lens rendering" spells it out): the thin lens's aperture sample and the point door's
// cosine-weighted direction both take it
TD void concentric_disk ( float l1, float l2, float& u, float& v ) {
    const float kPi2 = tdm_float ( 0x3FC90FDBu ), kPi4 = tdm_float ( 0x3F490FDBu );
    const float a = 2 * l1 - 1, b = 2 * l2 - 1;
    u = 0.f; v = 0.f;
    if ( ! ( a == 0.f && b == 0.f ) ) {
        float r, phi;
        if ( fabsf ( a ) > fabsf ( b ) ) { r = a; phi = kPi4 * ( b / a ); }
        else { r = b; phi = kPi2 - kPi4 * ( a / b ); }
        float sp, cp; tdm_sincosf_pair ( phi, sp, cp );          // (each bit-identical to tdm_sinf / tdm_cosf: dev_math.h)
        u = r * cp; v = r * sp;
    }
}

// The ray of a lens launch's sample (include/terra_amd.h "Lens rendering" is the definition): the one generator of the render kernels' lens instances,
// the lens AOV kernel and the unit entry. (l1, l2): the lens pair, looked at only where lens_draws -- the caller draws it from stream A then, after the sampler
// integration's pair, and passes anything otherwise. L is a launch constant: every branch on it is wave-uniform.
TD bool lens_draws ( const DevLens& L ) { return L.model == 0 && L.lens_radius > 0.f; }
TD void lens_sample ( const DevRenderParams& p, const DevLens& L, uint32_t px, uint32_t py, float r1, float r2, float l1, float l2, V3& ro, V3& rd ) {
    const float kPi = tdm_float ( 0x40490FDBu ), kPi2 = tdm_float ( 0x3FC90FDBu );
    float sx, sy; camera_film ( p, px, py, r1, r2, sx, sy );
    const V3 pos = v3 ( p.cam_pos[0], p.cam_pos[1], p.cam_pos[2] );
    float Lx = 0.f, Ly = 0.f;          // the origin's offset in the lens / film plane (models 0 with a lens, 1)
    bool shifted = false;
    if ( L.model == 0 ) {
        const float fx = sx * p.aspect * p.tan_half_fov;
        const float fy = sy * p.tan_half_fov;
        const V3 d = normalize ( v3 ( fx, fy, 1.f ) );
        if ( L.lens_radius > 0.f ) {
            float u, v; concentric_disk ( l1, l2, u, v );
            Lx = L.lens_radius * u; Ly = L.lens_radius * v; shifted = true;
            const float t = L.focus_distance / d.z;
            const V3 F = v3 ( d.x * t, d.y * t, d.z * t );          // where the pinhole ray meets the plane in focus
            rd = camera_rotate ( p, normalize ( v3 ( F.x - Lx, F.y - Ly, F.z ) ) );
        } else rd = camera_rotate ( p, d );
    } else if ( L.model == 1 ) {
        Lx = ( sx * p.aspect ) * L.ortho_half; Ly = sy * L.ortho_half; shifted = true;
        rd = camera_rotate ( p, v3 ( 0.f, 0.f, 1.f ) );
    } else if ( L.model == 2 ) {
        const float phi = sx * kPi, theta = sy * kPi2;
        float st, ct, sp, cp; tdm_sincosf_pair ( theta, st, ct ); tdm_sincosf_pair ( phi, sp, cp );
        rd = camera_rotate ( p, v3 ( ct * sp, st, ct * cp ) );
    } else {
        const float ux = sx * p.aspect, uy = sy, rr = sqrtf ( ux * ux + uy * uy ), theta = rr * L.fisheye_half;
        if ( rr == 0.f ) rd = camera_rotate ( p, v3 ( 0.f, 0.f, 1.f ) );
        else { float st, ct; tdm_sincosf_pair ( theta, st, ct ); rd = camera_rotate ( p, v3 ( ( st * ux ) / rr, ( st * uy ) / rr, ct ) ); }
    }
    ro = shifted ? v3 ( pos.x + ( p.cam_rot[0] * Lx + p.cam_rot[1] * Ly ), pos.y + ( p.cam_rot[3] * Lx + p.cam_rot[4] * Ly ), pos.z + ( p.cam_rot[6] * Lx + p.cam_rot[7] * Ly ) ) : pos;
}

// The ray of a point launch's sample (include/terra_amd.h "Point rendering" is the definition): the one generator of the render kernels' point instances,
// the point AOV kernel and the unit entry. pos / nrm: the pixel's TerraAmdPoint as stored (the normal not normalised); (g1, g2): the pair the caller draws from
// stream A after the sampler integration's. S is a launch constant: the branch on it is wave-uniform.
// an inactive point traces nothing: a component that is not finite, or a normal whose squared length is 0 (exactly, or by underflow) or not finite
TD bool point_inactive ( V3 pos, V3 nrm ) {
    const bool finite = fabsf ( pos.x ) < INFINITY && fabsf ( pos.y ) < INFINITY && fabsf ( pos.z ) < INFINITY && fabsf ( nrm.x ) < INFINITY && fabsf ( nrm.y ) < INFINITY && fabsf ( nrm.z ) < INFINITY;      // (false for a NaN too)
    const float q = nrm.x * nrm.x + nrm.y * nrm.y + nrm.z * nrm.z;
    return !finite || ! ( q > 0.f && q < INFINITY );
}
TD void point_sample ( const DevPointSampling& S, V3 pos, V3 nrm, float g1, float g2, V3& ro, V3& rd ) {
    const V3 n = normalize ( nrm );
    // the branch-free orthonormal basis of Duff et al. 2017 (make_basis keeps the reference's unnormalised tangent, which would skew the distribution)
    const float s = copysignf ( 1.f, n.z );
    const float a = -1.f / ( s + n.z );
    const float b = ( n.x * n.y ) * a;
    const V3 t = v3 ( 1.f + ( s * ( n.x * n.x ) ) * a, s * b, ( -s ) * n.x );
    const V3 bt = v3 ( b, s + ( n.y * n.y ) * a, -n.y );
    float x, y, z;
    if ( S.distribution == 0 ) {
        concentric_disk ( g1, g2, x, y );
        z = sqrtf ( fmaxf ( 0.f, ( 1.f - x * x ) - y * y ) );
    } else {
        z = 1.f - 2 * g1;
        const float r = sqrtf ( fmaxf ( 0.f, 1.f - z * z ) );
        const float phi = tdm_float ( 0x40C90FDBu ) * g2;          // 2 PI
        float sp, cp; tdm_sincosf_pair ( phi, sp, cp );
        x = r * cp; y = r * sp;
    }
    rd = normalize ( v3 ( ( x * t.x + y * bt.x ) + z * n.x, ( x * t.y + y * bt.y ) + z * n.y, ( x * t.z + y * bt.z ) + z * n.z ) );
    ro = pos;
}

// -----------------------------------------------------------------------------
// slab test
// -----------------------------------------------------------------------------
TD bool ray_aabb ( const Ray& r, V3 bmin, V3 bmax, float* tmin_out, float* tmax_out ) {
    float t1 = ( bmin.x - r.o.x ) * r.inv.x;
    float t2 = ( bmax.x - r.o.x ) * r.inv.x;
    float tmin = sel_min ( t1, t2 ), tmax = sel_max ( t1, t2 );
    t1 = ( bmin.y - r.o.y ) * r.inv.y;
    t2 = ( bmax.y - r.o.y ) * r.inv.y;
    tmin = sel_max ( tmin, sel_min ( t1, t2 ) ); tmax = sel_min ( tmax, sel_max ( t1, t2 ) );
    t1 = ( bmin.z - r.o.z ) * r.inv.z;
    t2 = ( bmax.z - r.o.z ) * r.inv.z;
    tmin = sel_max ( tmin, sel_min ( t1, t2 ) ); tmax = sel_min ( tmax, sel_max ( t1, t2 ) );
    bool hit = tmax > sel_max ( tmin, 0.f );
    if ( tmin_out ) *tmin_out = tmin;
    if ( tmax_out ) *tmax_out = tmax;
    return hit;
}

// -----------------------------------------------------------------------------
// slab test of one child box. FAST is legal when every component of the ray's
// inverse direction is finite and non-zero: then no NaN can appear (boxes and
// origins are finite) and "a<b?a:b" differs from v_min_f32 only in the sign of a
// zero, which the final comparison cannot see. Otherwise the compare-select form of
// the reference runs (NaN order matters there).
// -----------------------------------------------------------------------------
template <bool FAST>
TD bool slab ( V3 bmin, V3 bmax, const Ray& r ) {
    float t1x = ( bmin.x - r.o.x ) * r.inv.x, t2x = ( bmax.x - r.o.x ) * r.inv.x;
    float t1y = ( bmin.y - r.o.y ) * r.inv.y, t2y = ( bmax.y - r.o.y ) * r.inv.y;
    float t1z = ( bmin.z - r.o.z ) * r.inv.z, t2z = ( bmax.z - r.o.z ) * r.inv.z;
    if ( FAST ) {
        float tmin = __builtin_fmaxf ( __builtin_fmaxf ( __builtin_fminf ( t1x, t2x ), __builtin_fminf ( t1y, t2y ) ), __builtin_fminf ( t1z, t2z ) );
        float tmax = __builtin_fminf ( __builtin_fminf ( __builtin_fmaxf ( t1x, t2x ), __builtin_fmaxf ( t1y, t2y ) ), __builtin_fmaxf ( t1z, t2z ) );
        return tmax > __builtin_fmaxf ( tmin, 0.f );
    }
    float tmin = sel_min ( t1x, t2x ), tmax = sel_max ( t1x, t2x );
    tmin = sel_max ( tmin, sel_min ( t1y, t2y ) ); tmax = sel_min ( tmax, sel_max ( t1y, t2y ) );
    tmin = sel_max ( tmin, sel_min ( t1z, t2z ) ); tmax = sel_min ( tmax, sel_max ( t1z, t2z ) );
    return tmax > sel_max ( tmin, 0.f );
}

TD bool ray_is_regular ( const Ray& r ) {
    // finite and non-zero inverse direction components
    uint32_t ax = tdm_bits ( r.inv.x ) & 0x7fffffffu, ay = tdm_bits ( r.inv.y ) & 0x7fffffffu, az = tdm_bits ( r.inv.z ) & 0x7fffffffu;
    return ax - 1u < 0x7f7fffffu && ay - 1u < 0x7f7fffffu && az - 1u < 0x7f7fffffu;
}

// regular AND every |inverse direction component| below 2^96: origin * inv cannot overflow for any origin the containment check admits
TD bool ray_is_tame ( const Ray& r ) {
    uint32_t ax = tdm_bits ( r.inv.x ) & 0x7fffffffu, ay = tdm_bits ( r.inv.y ) & 0x7fffffffu, az = tdm_bits ( r.inv.z ) & 0x7fffffffu;
    return ax - 1u < 0x6f7fffffu && ay - 1u < 0x6f7fffffu && az - 1u < 0x6f7fffffu;
}
// One range test per ray (the kernels of ray_start_masks_for, their camera and continuation rays). make_ray_guarded's guard has already looked at the three numbers
// these two functions look at the reciprocals of: a direction component that passed xd_rcp_ok is normal with 2^-60 <= |d| <= 2^60, so RN ( 1 / d ) lies in
// [2^-60, 2^60] -- bits 0x21800000 .. 0x5d800000 without the sign, inside both 1 .. 0x7f7fffff (regular) and 1 .. 0x6f7fffff (tame). A wave whose lanes all passed
// the guard is therefore all tame and all regular, and the traversal entry (traverse_ref.h bvh_traverse_from) asks that first: "all_guarded || __all ( tame )" has
// the value of "__all ( tame )" for every input, and the second operand -- the three ands, the three decrements, the max and the vote -- runs only in a wave that
// holds a lane the guard turned away (a zero, a denormal, a huge, tiny or non-finite component, a significand of all ones), where it decides as it always did.
// slab test from (near, far) planes per axis: what slab<true> computes, without the per-axis min / max
TD bool slab_near_far ( float nx, float fx, float ny, float fy, float nz, float fz, const Ray& r ) {
    float tnx = ( nx - r.o.x ) * r.inv.x, tfx = ( fx - r.o.x ) * r.inv.x;
    float tny = ( ny - r.o.y ) * r.inv.y, tfy = ( fy - r.o.y ) * r.inv.y;
    float tnz = ( nz - r.o.z ) * r.inv.z, tfz = ( fz - r.o.z ) * r.inv.z;
    float tmin = __builtin_fmaxf ( __builtin_fmaxf ( tnx, tny ), tnz );
    float tmax = __builtin_fminf ( __builtin_fminf ( tfx, tfy ), tfz );
    return tmax > __builtin_fmaxf ( tmin, 0.f );
}

// The same test with t = fma ( plane, inv, -(o * inv) ): one instruction per plane instead of two. NOT the reference's arithmetic -- (plane - o) * inv -- so only the
// launches that need not reproduce the reference's traversal decision by decision may use it: the leaf-box-cull launches (Tracer::cull), whose commit-time proof
// (scene_host.cpp "numeric containment check") only asks that every box test be CONSERVATIVE within the error budget: a triangle the ray hits must pass the test of
// every box built around it. Here t carries two roundings -- of o * inv and of the fma -- worth u |o| + u |plane - o| in position, less than the three roundings of
// the reference form the budget was drawn up for. Which nodes are visited beyond that may differ from the replica's by a few per billion (never the image).
TD bool slab_near_far_fused ( float nx, float fx, float ny, float fy, float nz, float fz, const Ray& r, V3 oi, float& t_enter ) {
    float tnx = __builtin_fmaf ( nx, r.inv.x, -oi.x ), tfx = __builtin_fmaf ( fx, r.inv.x, -oi.x );
    float tny = __builtin_fmaf ( ny, r.inv.y, -oi.y ), tfy = __builtin_fmaf ( fy, r.inv.y, -oi.y );
    float tnz = __builtin_fmaf ( nz, r.inv.z, -oi.z ), tfz = __builtin_fmaf ( fz, r.inv.z, -oi.z );
    float tmin = __builtin_fmaxf ( __builtin_fmaxf ( tnx, tny ), tnz );
    float tmax = __builtin_fminf ( __builtin_fminf ( tfx, tfy ), tfz );
    t_enter = __builtin_fmaxf ( tmin, 0.f );
    return tmax > t_enter;
}

// -----------------------------------------------------------------------------
// watertight ray/triangle
// -----------------------------------------------------------------------------
TD RayState ray_state_init ( const Ray& r ) {
    float ax = fabsf ( r.d.x ), ay = fabsf ( r.d.y ), az = fabsf ( r.d.z );
    int iz = ax > ay ? ( ax > az ? 0 : 2 ) : ( ay > az ? 1 : 2 );   // ties -> later axis
    int ix = iz + 1 == 3 ? 0 : iz + 1;
    int iy = ix + 1 == 3 ? 0 : ix + 1;
    if ( pick ( r.d, iz ) < 0.f ) { int t = ix; ix = iy; iy = t; }
    RayState s;
    s.scalez = pick ( r.inv, iz );          // 1.f / d[iz] (src/TerraGeometry.c:124): the quotient make_ray already holds, same operands, same rounding
    s.shearx = pick ( r.d, ix ) * s.scalez;
    s.sheary = pick ( r.d, iy ) * s.scalez;
    s.ix = ix; s.iy = iy; s.iz = iz;
    return s;
}

// The same ray state, and the origin in the ray's axes, for the launches of ray_start_masks_for below: the axes as three lane predicates instead of three numbers --
// z0 / z1 = "iz is 0 / 1" (neither: 2), from the three comparisons above with ties to the later axis and a NaN losing every comparison it is in; flip = "d[iz] < 0"
// (false for -0 and a NaN). ix = iz + 1 and iy = iz + 2 (mod 3) change places when flip holds, so a pick is selects on masks that are already there: two for the
// component at iz, two each for those at iz + 1 and iz + 2, two more to put that pair in order -- 18 for d, inv and the origin. (Picking by the numbers, the
// compiler builds them with selects, additions and compares and compares them with 0 and 1 again at every pick: about 44 instructions.) The predicates do not
// leave this function. What the traversal needs later is a NUMBER -- perm for the ranked copy, the word offsets of tri_perm_lds -- and it is made here, in one
// vector register the empty asm pins: left alone the compiler makes perm where it is used, behind the box loop, and carries three masks there, which this
// kernel pays for with launch constants parked in vector lanes (profiles/ray_start/kernel_resources.md). ix, iy, iz come from perm by two 12-bit tables
// (ix = 1 2 2 0 0 1, iy = 2 1 0 2 1 0 for perm = 0 .. 5); only the launches without ranked copies read them.
// tests/test_ray_start.py restates both forms and holds them equal on every direction of {+-0, +-denormal, +-1, +-nextafter(1), +-2, +-inf, NaN}^3.
TD RayStateMasks ray_start_masks ( const Ray& r, V3& o_perm ) {
    const float ax = fabsf ( r.d.x ), ay = fabsf ( r.d.y ), az = fabsf ( r.d.z );
    const bool xy = ax > ay, xz = ax > az, yz = ay > az;
    const bool z0 = xy & xz, z1 = !xy & yz;
    const auto at_z = [&] ( V3 a ) { return z0 ? a.x : ( z1 ? a.y : a.z ); };
    const bool flip = at_z ( r.d ) < 0.f;
    const auto at_xy = [&] ( V3 a, float& px, float& py ) {
        const float u = z0 ? a.y : ( z1 ? a.z : a.x ), v = z0 ? a.z : ( z1 ? a.x : a.y );
        px = flip ? v : u; py = flip ? u : v;
    };
    RayStateMasks s;
    s.perm = ( z0 ? 0u : ( z1 ? 2u : 4u ) ) + ( flip ? 1u : 0u );
    asm volatile ( "" : "+v" ( s.perm ) );
    s.ix = ( int ) ( ( 0x429u >> ( 2u * s.perm ) ) & 3u ); s.iy = ( int ) ( ( 0x186u >> ( 2u * s.perm ) ) & 3u ); s.iz = ( int ) ( s.perm >> 1 );
    s.scalez = at_z ( r.inv );              // 1.f / d[iz], as ray_state_init takes it
    float dix, diy; at_xy ( r.d, dix, diy );
    s.shearx = dix * s.scalez;
    s.sheary = diy * s.scalez;
    at_xy ( r.o, o_perm.x, o_perm.y ); o_perm.z = at_z ( r.o );
    return s;
}
// Which launches start their rays that way and make one range test per ray (make_ray_guarded): the LDS-resident kernels of the plain presets without work counters, camera rays made in the kernel -- the headline's and Direct's kernels.
// Every other instance starts its rays with ray_state_init's integer selection of the axes and keeps both range tests: with the predicate form some of them took a few bytes more scratch
// (work-counter instances, MODE 0 light integrators, MODE 3), and the hall (MODE 2, a ray's state kept across the calls of a resumable loop) lost 1 %.
#if TERRA_RAY_SOURCE
#define TERRA_RAY_START_CAMERA 0
#else
#define TERRA_RAY_START_CAMERA 1
#endif
TD constexpr bool ray_start_masks_for ( int COUNT, int MODE, int KINDS ) { return TERRA_RAY_START_CAMERA && MODE == 1 && COUNT == 0 && KINDS == 1; }
// the camera sample of a render kernel: those kernels take the staged form (camera_sample_staged), every other one camera_sample
template <bool STAGED> TD V3 camera_direction ( const DevRenderParams& p, uint32_t px, uint32_t py, float r1, float r2 ) {
    if constexpr ( STAGED ) return camera_sample_staged ( p, px, py, r1, r2 ); else return camera_sample ( p, px, py, r1, r2 );
}

// the three vertices of a triangle record (three float4; the w components carry object, triangle in object, pad / rank)
TD void tri_vertices ( float4 t0, float4 t1, float4 t2, V3& a, V3& b, V3& c ) { a = v3 ( t0.x, t0.y, t0.z ); b = v3 ( t1.x, t1.y, t1.z ); c = v3 ( t2.x, t2.y, t2.z ); }
TD void tri_vertices ( const float4* tris, uint32_t i, V3& a, V3& b, V3& c ) { tri_vertices ( tris[3 * i], tris[3 * i + 1], tris[3 * i + 2], a, b, c ); }

// A triangle in the ray's permuted axes: a[0..2] = vertex a [ix], [iy], [iz], likewise b and c. Two loaders: from the 12-float record the block
// staged in LDS (a.xyz object | b.xyz triangle-in-object | c.xyz pad), which reads the components it needs by index, and from the record's three
// float4 out of global memory, which selects them in registers.
struct TriPerm { float a[3], b[3], c[3]; };
TD TriPerm tri_perm_lds ( const float* t, const RayState& s ) {
    TriPerm p;
    p.a[0] = t[s.ix]; p.a[1] = t[s.iy]; p.a[2] = t[s.iz];
    p.b[0] = t[4 + s.ix]; p.b[1] = t[4 + s.iy]; p.b[2] = t[4 + s.iz];
    p.c[0] = t[8 + s.ix]; p.c[1] = t[8 + s.iy]; p.c[2] = t[8 + s.iz];
    return p;
}
TD TriPerm tri_perm ( float4 t0, float4 t1, float4 t2, const RayState& s ) {
    const V3 va = v3 ( t0.x, t0.y, t0.z ), vb = v3 ( t1.x, t1.y, t1.z ), vc = v3 ( t2.x, t2.y, t2.z );
    TriPerm p;
    p.a[0] = pick ( va, s.ix ); p.a[1] = pick ( va, s.iy ); p.a[2] = pick ( va, s.iz );
    p.b[0] = pick ( vb, s.ix ); p.b[1] = pick ( vb, s.iy ); p.b[2] = pick ( vb, s.iz );
    p.c[0] = pick ( vc, s.ix ); p.c[1] = pick ( vc, s.iy ); p.c[2] = pick ( vc, s.iz );
    return p;
}

struct TriHit { float u, v, w, depth; V3 point; };

TD bool watertight ( const Ray& r, const RayState& s, V3 ta, V3 tb, V3 tc, TriHit& h ) {
    V3 A = ta - r.o, B = tb - r.o, C = tc - r.o;
    float Aiz = pick ( A, s.iz ), Biz = pick ( B, s.iz ), Ciz = pick ( C, s.iz );
    float Ax = pick ( A, s.ix ) - s.shearx * Aiz, Ay = pick ( A, s.iy ) - s.sheary * Aiz;
    float Bx = pick ( B, s.ix ) - s.shearx * Biz, By = pick ( B, s.iy ) - s.sheary * Biz;
    float Cx = pick ( C, s.ix ) - s.shearx * Ciz, Cy = pick ( C, s.iy ) - s.sheary * Ciz;
    float U = Cx * By - Cy * Bx;
    float V = Ax * Cy - Ay * Cx;
    float W = Bx * Ay - By * Ax;
    if ( U == 0.f || V == 0.f || W == 0.f ) {
        U = ( float ) ( ( double ) Cx * ( double ) By - ( double ) Cy * ( double ) Bx );
        V = ( float ) ( ( double ) Ax * ( double ) Cy - ( double ) Ay * ( double ) Cx );
        W = ( float ) ( ( double ) Bx * ( double ) Ay - ( double ) By * ( double ) Ax );
    }
    uint32_t sign = tdm_bits ( U ) & 0x80000000u;
    if ( ( ( tdm_bits ( V ) ^ tdm_bits ( U ) ) | ( tdm_bits ( W ) ^ tdm_bits ( U ) ) ) & 0x80000000u ) return false;
    float det = U + V + W;
    if ( det == 0.f ) return false;
    float Az = s.scalez * Aiz, Bz = s.scalez * Biz, Cz = s.scalez * Ciz;
    float depth = U * Az + V * Bz + W * Cz;
    if ( tdm_float ( tdm_bits ( depth ) ^ sign ) < 0.f ) return false;
    float inv_det = 1.f / det;
    h.u = U * inv_det; h.v = V * inv_det; h.w = W * inv_det;
    h.depth = depth * inv_det;
    h.point = r.o + r.d * h.depth;
    return true;
}

// -----------------------------------------------------------------------------
// watertight test on components already gathered in the ray's permuted axes
// (TriPerm); o = origin permuted the same way.
// Same operations, in the same order, as watertight() above.
// -----------------------------------------------------------------------------
TD bool watertight_permuted ( const TriPerm& t, V3 o, const RayState& s, float& depth_out ) {
    float Aix = t.a[0] - o.x, Aiy = t.a[1] - o.y, Aiz = t.a[2] - o.z;
    float Bix = t.b[0] - o.x, Biy = t.b[1] - o.y, Biz = t.b[2] - o.z;
    float Cix = t.c[0] - o.x, Ciy = t.c[1] - o.y, Ciz = t.c[2] - o.z;
    float Ax = Aix - s.shearx * Aiz, Ay = Aiy - s.sheary * Aiz;
    float Bx = Bix - s.shearx * Biz, By = Biy - s.sheary * Biz;
    float Cx = Cix - s.shearx * Ciz, Cy = Ciy - s.sheary * Ciz;
    float U = Cx * By - Cy * Bx;
    float V = Ax * Cy - Ay * Cx;
    float W = Bx * Ay - By * Ax;
    if ( U == 0.f || V == 0.f || W == 0.f ) {
        U = ( float ) ( ( double ) Cx * ( double ) By - ( double ) Cy * ( double ) Bx );
        V = ( float ) ( ( double ) Ax * ( double ) Cy - ( double ) Ay * ( double ) Cx );
        W = ( float ) ( ( double ) Bx * ( double ) Ay - ( double ) By * ( double ) Ax );
    }
    uint32_t sign = tdm_bits ( U ) & 0x80000000u;
    if ( ( ( tdm_bits ( V ) ^ tdm_bits ( U ) ) | ( tdm_bits ( W ) ^ tdm_bits ( U ) ) ) & 0x80000000u ) return false;
    float det = U + V + W;
    if ( det == 0.f ) return false;
    float Az = s.scalez * Aiz, Bz = s.scalez * Biz, Cz = s.scalez * Ciz;
    float depth = U * Az + V * Bz + W * Cz;
    if ( tdm_float ( tdm_bits ( depth ) ^ sign ) < 0.f ) return false;
    float inv_det = 1.f / det;
    depth_out = depth * inv_det;
    return true;
}

// -----------------------------------------------------------------------------
// watertight test of a PAIR of triangles that share an edge as a fan does: T1 = (p0, p1, p2), T2 = (p0, p2, p3), components already in the ray's permuted axes.
// Per triangle the same operations, in the same order, as watertight_permuted -- so the same answer and the same depth bit for bit -- with what the two share done once:
//   * the four vertices are translated and sheared once;
//   * the diagonal's edge function: V of T1 = p0.x p2.y - p0.y p2.x, W of T2 = p2.x p0.y - p2.y p0.x -- the same two products (a product does not depend on the order of
//     its factors) subtracted the other way round, and in round-to-nearest b - a = -(a - b) exactly, up to the sign of a zero: W2 = -V1 whenever V1 != 0;
//   * the part after the sign test (determinant, depth and its sign, the division) runs once, for the triangle the lane's sign test passed: a ray through a quad
//     passes at most one of the two except on the diagonal or in a folded pair, and only where some lane of the wave passes both does the part run again, for T2.
// A triangle with an edge function that is +-0 takes the double-precision fallback, each triangle by its own zero test (V1 = +-0 sends both: W2 is +-0 then). That
// triangle leaves the shared path and is tested afterwards by watertight_permuted itself, from vertices read AGAIN -- so the rare fallback's registers are not live
// beside the pair's twelve components; the other triangle of the pair stays on the shared path with its float values untouched.
// load ( again ): the pair's vertices (again: the second read; the loader hides from the optimiser that it is the same address, which would keep the first copy alive).
// record ( depth, second ) is called for each triangle hit (second: T2), in no particular order.
// -----------------------------------------------------------------------------
struct PairPerm { float p0[3], p1[3], p2[3], p3[3]; };
TD bool pair_finish ( float U, float V, float W, float Aiz, float Biz, float Ciz, const RayState& s, float& depth_out ) {
    uint32_t sign = tdm_bits ( U ) & 0x80000000u;
    float det = U + V + W;
    if ( det == 0.f ) return false;
    float Az = s.scalez * Aiz, Bz = s.scalez * Biz, Cz = s.scalez * Ciz;
    float depth = U * Az + V * Bz + W * Cz;
    if ( tdm_float ( tdm_bits ( depth ) ^ sign ) < 0.f ) return false;
    float inv_det = 1.f / det;
    depth_out = depth * inv_det;
    return true;
}
template <class Load, class Record>
TD void watertight_pair ( Load&& load, V3 o, const RayState& s, Record&& record ) {
    bool z1, z2;          // T1 / T2 has an edge function that is +-0
    {
        const PairPerm t = load ( false );
        float P0ix = t.p0[0] - o.x, P0iy = t.p0[1] - o.y, P0iz = t.p0[2] - o.z;
        float P1ix = t.p1[0] - o.x, P1iy = t.p1[1] - o.y, P1iz = t.p1[2] - o.z;
        float P2ix = t.p2[0] - o.x, P2iy = t.p2[1] - o.y, P2iz = t.p2[2] - o.z;
        float P3ix = t.p3[0] - o.x, P3iy = t.p3[1] - o.y, P3iz = t.p3[2] - o.z;
        float P0x = P0ix - s.shearx * P0iz, P0y = P0iy - s.sheary * P0iz;
        float P1x = P1ix - s.shearx * P1iz, P1y = P1iy - s.sheary * P1iz;
        float P2x = P2ix - s.shearx * P2iz, P2y = P2iy - s.sheary * P2iz;
        float P3x = P3ix - s.shearx * P3iz, P3y = P3iy - s.sheary * P3iz;
        // T1: A = p0, B = p1, C = p2;  T2: A = p0, B = p2, C = p3
        float U1 = P2x * P1y - P2y * P1x;
        float V1 = P0x * P2y - P0y * P2x;
        float W1 = P1x * P0y - P1y * P0x;
        float U2 = P3x * P2y - P3y * P2x;
        float V2 = P0x * P3y - P0y * P3x;
        float W2 = -V1;
        z1 = U1 == 0.f || V1 == 0.f || W1 == 0.f;
        z2 = U2 == 0.f || V2 == 0.f || V1 == 0.f;
        const bool pass1 = !z1 && ! ( ( ( tdm_bits ( V1 ) ^ tdm_bits ( U1 ) ) | ( tdm_bits ( W1 ) ^ tdm_bits ( U1 ) ) ) & 0x80000000u );
        const bool pass2 = !z2 && ! ( ( ( tdm_bits ( V2 ) ^ tdm_bits ( U2 ) ) | ( tdm_bits ( W2 ) ^ tdm_bits ( U2 ) ) ) & 0x80000000u );
        if ( pass1 || pass2 ) {          // the triangle that passed (T1 where both did) through the one copy of the rest
            float depth;
            if ( pair_finish ( pass1 ? U1 : U2, pass1 ? V1 : V2, pass1 ? W1 : W2, P0iz, pass1 ? P1iz : P2iz, pass1 ? P2iz : P3iz, s, depth ) ) record ( depth, !pass1 );
        }
        if ( __any ( pass1 && pass2 ) ) {          // on the diagonal, or a folded pair: T2 of the lanes that had T1 above
            float depth;
            if ( pass1 && pass2 && pair_finish ( U2, V2, W2, P0iz, P2iz, P3iz, s, depth ) ) record ( depth, true );
        }
    }
    if ( z1 ) {
        const PairPerm t = load ( true );
        const TriPerm tp = { { t.p0[0], t.p0[1], t.p0[2] }, { t.p1[0], t.p1[1], t.p1[2] }, { t.p2[0], t.p2[1], t.p2[2] } };
        float depth;
        if ( watertight_permuted ( tp, o, s, depth ) ) record ( depth, false );
    }
    if ( z2 ) {
        const PairPerm t = load ( true );
        const TriPerm tp = { { t.p0[0], t.p0[1], t.p0[2] }, { t.p2[0], t.p2[1], t.p2[2] }, { t.p3[0], t.p3[1], t.p3[2] } };
        float depth;
        if ( watertight_permuted ( tp, o, s, depth ) ) record ( depth, true );
    }
}

TD bool moller_trumbore ( V3 o, V3 d, V3 ta, V3 tb, V3 tc, float& t_out, V3& p_out ) {
    V3 e1 = tb - ta, e2 = tc - ta;
    V3 h = cross ( d, e2 );
    float a = dot ( e1, h );
    if ( ( double ) a > -1e-4 && ( double ) a < 1e-4 ) return false;
    float f = 1 / a;
    V3 s = o - ta;
    float u = f * dot ( s, h );
    if ( u < 0.f || u > 1.f ) return false;
    V3 q = cross ( s, e1 );
    float v = f * dot ( d, q );
    if ( v < 0.f || u + v > 1.f ) return false;
    float t = f * dot ( e2, q );
    if ( t > 0.00001f ) { t_out = t; p_out = d * t + o; return true; }
    return false;
}
