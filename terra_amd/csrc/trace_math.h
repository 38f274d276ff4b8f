// trace_math.h -- bottom layer of the device hot path (trace_device.h lists the layers): vectors, the shading basis, rays and the
// per-ray state of the watertight test.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include "dev_types.h"
#include "dev_math.h"
#include "rng.h"
#include "sampling_device.h"
#include "exact_div.h"
#include "exact_sqrt.h"

#define TD __device__ __forceinline__

struct V3 { float x, y, z; };

TD V3 v3 ( float x, float y, float z ) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
TD V3 v3p ( const float* p ) { return v3 ( p[0], p[1], p[2] ); }
TD V3 operator+ ( V3 a, V3 b ) { return v3 ( a.x + b.x, a.y + b.y, a.z + b.z ); }
TD V3 operator- ( V3 a, V3 b ) { return v3 ( a.x - b.x, a.y - b.y, a.z - b.z ); }
TD V3 operator* ( V3 a, float s ) { return v3 ( a.x * s, a.y * s, a.z * s ); }
TD V3 had ( V3 a, V3 b ) { return v3 ( a.x * b.x, a.y * b.y, a.z * b.z ); }
TD V3 neg ( V3 a ) { return v3 ( -a.x, -a.y, -a.z ); }
TD float dot ( V3 a, V3 b ) { return a.x * b.x + a.y * b.y + a.z * b.z; }
TD V3 cross ( V3 a, V3 b ) { return v3 ( a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x ); }
TD float length2 ( V3 a ) { return a.x * a.x + a.y * a.y + a.z * a.z; }
TD float length ( V3 a ) { return sqrtf ( length2 ( a ) ); }          // (the plain root: its callers are the denoise, temporal and AOV kernels and one-off sites)
// a / |a|: the short root of the squared length (exact_sqrt.h), then three quotients that share one refined reciprocal of the length (exact_div.h), each behind its
// own guard; normalize_plain is the same function written with sqrtf and "/" (the unit entries compare them)
TD V3 normalize_plain ( V3 a ) { float l = sqrtf ( length2 ( a ) ); return v3 ( a.x / l, a.y / l, a.z / l ); }
// (normalize_site below restates normalize for the shading stages, make_basis_site restates make_basis: a change of either goes into both)
TD V3 normalize ( V3 a ) { float l = sqrt_exact ( length2 ( a ) ); V3 r; xd_normalize3 ( a.x, a.y, a.z, l, r.x, r.y, r.z ); return r; }
// normalize as two sites of a shading stage (exact_div.h "Shading stages"): SHORT = false is normalize itself
template <bool SHORT> TD V3 normalize_site ( V3 a, int& ok ) {
    const float l2 = length2 ( a ), l = xs_site_sqrt<SHORT> ( l2, xs_in_range ( l2 ), ok );
    V3 r; xd_site_normalize3<SHORT> ( a.x, a.y, a.z, l, r.x, r.y, r.z, ok ); return r;
}
// compare-selects: exactly "a < b ? a : b" / "a > b ? a : b" (NaN-order sensitive)
TD float sel_min ( float a, float b ) { return a < b ? a : b; }
TD float sel_max ( float a, float b ) { return a > b ? a : b; }
TD float pick ( V3 a, int i ) { return i == 0 ? a.x : ( i == 1 ? a.y : a.z ); }

// columns of the shading basis: tangent, normal, bitangent. Stored by rows as the reference does.
struct Basis { float r0[3], r1[3], r2[3]; };
TD V3 basis_apply ( const Basis& m, V3 v ) {
    return v3 ( m.r0[0] * v.x + m.r0[1] * v.y + m.r0[2] * v.z,
                m.r1[0] * v.x + m.r1[1] * v.y + m.r1[2] * v.z,
                m.r2[0] * v.x + m.r2[1] * v.y + m.r2[2] * v.z );
}
TD Basis basis_of ( V3 t, V3 n ) {
    V3 b = cross ( n, t );
    Basis m;
    m.r0[0] = t.x; m.r0[1] = n.x; m.r0[2] = b.x;
    m.r1[0] = t.y; m.r1[1] = n.y; m.r1[2] = b.y;
    m.r2[0] = t.z; m.r2[1] = n.z; m.r2[2] = b.z;
    return m;
}
// the tangent as the reference writes it: two arms, a root and three products in each (the unit entry compares make_basis with it)
TD Basis make_basis_plain ( V3 n ) {
    V3 t;
    if ( fabsf ( n.x ) > fabsf ( n.y ) ) {
        float k = sqrtf ( n.x * n.x + n.z * n.z );
        t = v3 ( n.z * k, 0.f * k, -n.x * k );
    } else {
        float k = sqrtf ( n.y * n.y + n.z * n.z );
        t = v3 ( 0.f * k, -n.z * k, n.y * k );
    }
    return basis_of ( t, n );
}
// ... and as the kernels run it: the arms are one computation on different operands, so the operands are selected and one path runs -- a wave whose lanes disagree
// on the comparison no longer executes both arms. Same sum order, same three products, the negations on the operands as above; the products by 0.f stay (k may be
// NaN or inf)
TD Basis make_basis ( V3 n ) {
    const bool c = fabsf ( n.x ) > fabsf ( n.y );
    const float a = c ? n.x : n.y;
    const float k = sqrt_exact ( a * a + n.z * n.z );
    return basis_of ( v3 ( ( c ? n.z : 0.f ) * k, ( c ? 0.f : -n.z ) * k, ( c ? -n.x : n.y ) * k ), n );
}
// ... as a site of a shading stage: SHORT = false is make_basis itself
template <bool SHORT> TD Basis make_basis_site ( V3 n, int& ok ) {
    const bool c = fabsf ( n.x ) > fabsf ( n.y );
    const float a = c ? n.x : n.y;
    const float kk = a * a + n.z * n.z, k = xs_site_sqrt<SHORT> ( kk, xs_in_range ( kk ), ok );
    return basis_of ( v3 ( ( c ? n.z : 0.f ) * k, ( c ? 0.f : -n.z ) * k, ( c ? -n.x : n.y ) * k ), n );
}

struct Ray { V3 o, d, inv; };
TD Ray make_ray ( V3 o, V3 d ) { Ray r; r.o = o; r.d = d; rcp3_exact ( d.x, d.y, d.z, r.inv.x, r.inv.y, r.inv.z ); return r; }      // 1.f / d, bit for bit -- 1 / -0 = -inf included: a zero takes the plain division
// make_ray that also says what its guard found (the kernels of trace_geometry.h ray_start_masks_for): guarded = every component of d passed xd_rcp_ok, so inv came
// from the short sequence. Such a component is normal with 2^-60 <= |d| <= 2^60, and its correctly rounded reciprocal lies in [2^-60, 2^60] too (rounding is
// monotonic and both bounds are floats): finite, non-zero and far below 2^96 -- the ray is regular and tame (trace_geometry.h ray_is_regular, ray_is_tame)
// without looking at inv again. tests/test_ray_start.py holds the implication on the bits. Same quotients as make_ray, bit for bit.
TD Ray make_ray_guarded ( V3 o, V3 d, bool& guarded ) {
    Ray r; r.o = o; r.d = d;
    guarded = ( xd_rcp_ok ( d.x ) & xd_rcp_ok ( d.y ) & xd_rcp_ok ( d.z ) ) != 0;
    if ( guarded ) { r.inv.x = xd_rcp_short ( d.x ); r.inv.y = xd_rcp_short ( d.y ); r.inv.z = xd_rcp_short ( d.z ); }
    else { r.inv.x = 1.f / d.x; r.inv.y = 1.f / d.y; r.inv.z = 1.f / d.z; }
    return r;
}
// Stage S1 of the shading stages (exact_div.h "Shading stages"), the next ray's three reciprocals. Returns the lane's mask: every component passed its guard --
// make_ray_guarded's `guarded`. SHORT: the short sequences run unguarded and the caller votes; otherwise make_ray_guarded's own lines. DROPS: d is a camera or
// continuation direction of a launch whose constants passed terra_camera_stage_limits (dev_types.h), and its components need no upper bound (xd_rcp_unit_ok;
// the argument stands beside it). `guarded` then still implies what the traversal entry derives from it (trace_geometry.h "One range test per ray"): the
// component is normal with 2^-60 <= |d| < 8, its reciprocal lies in ( 2^-3, 2^60 ].
#ifndef TERRA_SHADE_STAGES         // (A/B) 1: the kernels of ray_start_masks_for shade in stages, one fallback vote per stage; 0: every site keeps its own branch
#define TERRA_SHADE_STAGES 1
#endif
#ifndef TERRA_SHADE_DROPS          // (A/B) 1: those kernels leave out the range tests their data cannot fail; 0: every site keeps its whole guard
#define TERRA_SHADE_DROPS 1
#endif
template <bool SHORT, bool DROPS> TD int ray_stage ( V3 o, V3 d, Ray& r ) {
    r.o = o; r.d = d;
    const int ok = DROPS ? xd_rcp_unit_ok ( d.x ) & xd_rcp_unit_ok ( d.y ) & xd_rcp_unit_ok ( d.z ) : xd_rcp_ok ( d.x ) & xd_rcp_ok ( d.y ) & xd_rcp_ok ( d.z );
    if ( SHORT || ok ) { r.inv.x = xd_rcp_short ( d.x ); r.inv.y = xd_rcp_short ( d.y ); r.inv.z = xd_rcp_short ( d.z ); }
    else { r.inv.x = 1.f / d.x; r.inv.y = 1.f / d.y; r.inv.z = 1.f / d.z; }
    return ok;
}
// the stage as the render loop runs it: one vote; a wave that holds a lane the guard turned away takes make_ray_guarded, all of it
// s1_guarded: DevRenderParams::shade_s1_guarded, a launch constant -- a launch outside the camera limits keeps make_ray_guarded, every test with its own branch
TD Ray make_ray_staged ( V3 o, V3 d, bool& guarded, uint32_t s1_guarded ) {
    Ray r;
    if ( s1_guarded ) return make_ray_guarded ( o, d, guarded );
    if constexpr ( TERRA_SHADE_STAGES != 0 ) {
        guarded = ray_stage<true, TERRA_SHADE_DROPS != 0> ( o, d, r ) != 0;
        if ( __any ( !guarded ) ) r = make_ray_guarded ( o, d, guarded );
    } else guarded = ray_stage<false, TERRA_SHADE_DROPS != 0> ( o, d, r ) != 0;
    return r;
}

// what the watertight test keeps per ray (ray_state_init): the dominant axis iz of the direction, the two others in winding order, the shear and the scale
struct RayState { float shearx, sheary, scalez; int ix, iy, iz; };
// a point in the ray's permuted axes: (a[ix], a[iy], a[iz])
TD V3 permuted ( V3 a, const RayState& s ) { return v3 ( pick ( a, s.ix ), pick ( a, s.iy ), pick ( a, s.iz ) ); }
// which of the six pre-permuted copies of the ranked triangles the ray reads (scene_host.cpp): 2 iz + "ix does not follow iz" (d[iz] < 0 swapped ix / iy)
TD uint32_t ray_perm ( const RayState& s ) { return 2u * ( uint32_t ) s.iz + ( uint32_t ) ( s.ix != ( s.iz == 2 ? 0 : s.iz + 1 ) ); }
// the ray state of trace_geometry.h ray_start_masks: that number is made at the ray's start and kept
struct RayStateMasks : RayState { uint32_t perm; };
TD uint32_t ray_perm ( const RayStateMasks& s ) { return s.perm; }
