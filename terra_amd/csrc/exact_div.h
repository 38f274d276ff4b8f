// exact_div.h -- correctly rounded float quotients in fewer instructions than the IEEE expansion of "/" (DESIGN.md 5 "Where the arithmetic legitimately differs",
// entry 4: the argument). Every helper returns the bits "/" returns, for every input: inside a guarded range it takes a short fma sequence that is proved to round as the
// division does (Markstein's theorems on a reciprocal refined by fma, and on a quotient corrected by one exact remainder), outside it it IS the plain "/", behind a branch.
//   rcp_exact ( d )               = 1.f / d
//   div_exact_r ( x, d, r )       = x / d, r = rcp_exact ( d ) or any correctly rounded 1 / d (a host's 1.f / d)
//   div_exact_rk ( x, d, r )      = x / d for a denominator the CALLER knows to be normal with 2^-60 <= |d| <= 2^60 (a launch constant, a literal)
//   div2_exact ( x1, x2, d, .. )  = x1 / d and x2 / d, one reciprocal; div2_exact_rk: two quotients by known denominators behind one branch
//   rcp3_exact ( .. )             = three reciprocals behind one branch (make_ray)
//   xd_normalize3 ( x, y, z, l, .. ) = x / l, y / l, z / l for l = the vector's length (>= 0 or NaN, as sqrtf returns it): one reciprocal, three quotients
//   roulette_scale ( pr )         = ( float ) ( 1.0 / ( ( double ) pr + 1e-4 ) ): the double division's own reciprocal and fma steps, without its scaling and fix-up
// The A/B against the plain "/" in every helper: profiles/exact_div/ab.md (roulette_scale: profiles/short_sqrt/ab.md).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define XD __device__ __forceinline__

// The guarded range of every operand: normal, 2^-60 <= |v| <= 2^60 (a NaN fails both comparisons). Then a quotient lies in [2^-120, 2^120], a reciprocal in
// [2^-60, 2^60], and the remainders below -- no smaller than 2^-48 times an operand product -- are normal too: nothing in a short sequence underflows, overflows or
// meets a denormal, which is all that the theorems (stated for an unbounded exponent range) ask of the format.
// (The guards are ints joined with "&", not bools with "&&": every comparison is evaluated and ONE branch chooses between the short sequence and the division.)
XD int xd_in_range ( float v ) { const float a = __builtin_fabsf ( v ); return ( int ) ( a >= 0x1p-60f ) & ( int ) ( a <= 0x1p60f ); }
// ... and, for a denominator whose reciprocal is refined here, a significand that is not all ones: the one pattern Markstein's reciprocal theorem excludes
// (1 / (2 - 2^-23) lies 2^-48 above a rounding midpoint, and the last fma can land on the midpoint itself)
XD int xd_rcp_ok ( float d ) { return xd_in_range ( d ) & ( int ) ( ( __float_as_uint ( d ) & 0x7fffffu ) != 0x7fffffu ); }

// v_rcp_f32 (1 ulp) and two Newton steps in fma: after the first the estimate is within a unit of the last place of 1 / d, where the residual 1 - d y is exact and the
// second step rounds 1 / d correctly (Markstein 1990, theorem on the reciprocal; significand of d not all ones). Checked on all 2^32 patterns (tests/test_exact_div_gpu.py).
XD float xd_rcp_short ( float d ) {
    float y = __builtin_amdgcn_rcpf ( d );
    float e = __builtin_fmaf ( -d, y, 1.f );
    y = __builtin_fmaf ( e, y, y );
    e = __builtin_fmaf ( -d, y, 1.f );
    return __builtin_fmaf ( e, y, y );
}
// r = RN ( 1 / d ): q0 = RN ( x r ) is within a unit of the last place of x / d, so rem = x - d q0 is exact, and RN ( q0 + rem r ) = RN ( x / d ) (Markstein's
// theorem on the quotient; no significand is excluded).
XD float xd_div_short ( float x, float d, float r ) {
    const float q0 = x * r;
    const float rem = __builtin_fmaf ( -d, q0, x );
    return __builtin_fmaf ( rem, r, q0 );
}
// the same for d > 0 and a numerator that may be +-0. The form above returns +0 for x = -0: its remainder is (+0) + (-0) = +0, and (+0) r + (-0) = +0. Here the
// remainder is formed negated, d q0 - x, and subtracted: for x = -0 it is (-0) + (+0) = +0 and the last fma adds (-0) r = -0 to q0 = -0: -0; for x = +0 it adds
// (-0) r = -0 to q0 = +0: +0 -- the quotient's own zero both times. For x != 0 the remainder is the same number, exactly.
XD float xd_div_short_pos ( float x, float d, float r ) {
    const float q0 = x * r;
    const float nrem = __builtin_fmaf ( d, q0, -x );
    return __builtin_fmaf ( -nrem, r, q0 );
}

XD float rcp_exact ( float d ) {
    if ( xd_rcp_ok ( d ) ) return xd_rcp_short ( d );
    return 1.f / d;
}
XD float div_exact_r ( float x, float d, float r ) {
    if ( xd_in_range ( x ) & xd_in_range ( d ) ) return xd_div_short ( x, d, r );
    return x / d;
}
XD float div_exact_rk ( float x, float d, float r ) {
    if ( xd_in_range ( x ) ) return xd_div_short ( x, d, r );
    return x / d;
}
// x1 / d, x2 / d for one such denominator, behind one branch
XD void div2_exact_rk ( float x1, float x2, float d1, float r1, float d2, float r2, float& q1, float& q2 ) {
    if ( xd_in_range ( x1 ) & xd_in_range ( x2 ) ) { q1 = xd_div_short ( x1, d1, r1 ); q2 = xd_div_short ( x2, d2, r2 ); return; }
    q1 = x1 / d1; q2 = x2 / d2;
}
XD void div2_exact ( float x1, float x2, float d, float& q1, float& q2 ) {
    if ( xd_rcp_ok ( d ) & xd_in_range ( x1 ) & xd_in_range ( x2 ) ) {
        const float r = xd_rcp_short ( d );
        q1 = xd_div_short ( x1, d, r ); q2 = xd_div_short ( x2, d, r );
        return;
    }
    q1 = x1 / d; q2 = x2 / d;
}
XD void rcp3_exact ( float dx, float dy, float dz, float& rx, float& ry, float& rz ) {
    if ( xd_rcp_ok ( dx ) & xd_rcp_ok ( dy ) & xd_rcp_ok ( dz ) ) { rx = xd_rcp_short ( dx ); ry = xd_rcp_short ( dy ); rz = xd_rcp_short ( dz ); return; }
    rx = 1.f / dx; ry = 1.f / dy; rz = 1.f / dz;
}
// a component of a vector of length l in the guarded range: +-0, or no smaller than 2^-60 (it cannot exceed l by more than a rounding, so it needs no upper bound)
XD int xd_component_ok ( float c ) { return ( int ) ( c == 0.f ) | ( int ) ( __builtin_fabsf ( c ) >= 0x1p-60f ); }
XD void xd_normalize3 ( float x, float y, float z, float l, float& qx, float& qy, float& qz ) {
    if ( ( int ) ( l >= 0x1p-60f ) & ( int ) ( l <= 0x1p60f ) & ( int ) ( ( __float_as_uint ( l ) & 0x7fffffu ) != 0x7fffffu ) & xd_component_ok ( x ) & xd_component_ok ( y ) & xd_component_ok ( z ) ) {          // (xd_rcp_ok for l > 0)
        const float r = xd_rcp_short ( l );
        qx = xd_div_short_pos ( x, l, r ); qy = xd_div_short_pos ( y, l, r ); qz = xd_div_short_pos ( z, l, r );
        return;
    }
    qx = x / l; qy = y / l; qz = z / l;
}

// The Russian-roulette rescale (integrators_device.h path_continue): ( float ) ( 1.0 / ( ( double ) pr + 1e-4 ) ), bit for bit. The IEEE expansion of the double
// division is v_div_scale (twice), v_rcp_f64, two Newton steps, q = n y, the remainder n - d q, v_div_fmas, v_div_fixup: 13 instructions. For 0 <= pr <= 2^60 the
// denominator lies in [1e-4, 2^60 + 1e-4]: both v_div_scale pass their operand through, the numerator 1.0 makes q = y exactly, v_div_fmas applies no scale and
// v_div_fixup meets no special operand -- what is left is the reciprocal, two Newton steps and the last correction e = 1 - d y, y + e y (Markstein's step), the same
// operations on the same operands: 7 instructions. Any other pr (negative, huge, NaN) takes the plain expression. All 2^32 patterns: tests/test_exact_sqrt_gpu.py.
// (its guard and its short arm on their own, for the shading stages below)
XD int roulette_scale_ok ( float pr ) { return ( int ) ( pr >= 0.f ) & ( int ) ( pr <= 0x1p60f ); }
XD float roulette_scale_short ( float pr ) {
    const double d = ( double ) pr + 1e-4;
    double y = __builtin_amdgcn_rcp ( d );
    double e = __builtin_fma ( -d, y, 1.0 ); y = __builtin_fma ( y, e, y );
    e = __builtin_fma ( -d, y, 1.0 ); y = __builtin_fma ( y, e, y );
    e = __builtin_fma ( -d, y, 1.0 ); y = __builtin_fma ( e, y, y );
    return ( float ) y;
}
XD float roulette_scale ( float pr ) {
    const double d = ( double ) pr + 1e-4;
    if ( ( int ) ( pr >= 0.f ) & ( int ) ( pr <= 0x1p60f ) ) {
        double y = __builtin_amdgcn_rcp ( d );
        double e = __builtin_fma ( -d, y, 1.0 ); y = __builtin_fma ( y, e, y );
        e = __builtin_fma ( -d, y, 1.0 ); y = __builtin_fma ( y, e, y );
        e = __builtin_fma ( -d, y, 1.0 ); y = __builtin_fma ( e, y, y );
        return ( float ) y;
    }
    return ( float ) ( 1.0 / d );
}

// ---- Shading stages (DESIGN.md 3.1 "Shading"): the kernels of trace_geometry.h ray_start_masks_for. A guarded helper above spends a branch per call site -- an exec
// save, a conditional branch and a join around every short sequence. A STAGE (trace_math.h ray_stage, shading_device.h surface_stage, integrators_device.h
// continue_stage) runs the short sequences of several sites unconditionally, ANDs the sites' guards -- the *_ok predicates of this file and of exact_sqrt.h -- into
// one lane mask and takes ONE wave vote: where any lane of the wave failed any site, the whole stage is computed again, for the whole wave, by the guarded helpers,
// before anything of it is used. A lane that passed every guard got from the short sequences the bits the guarded helpers return (they would have run those very
// sequences); a lane that failed gets the guarded helpers' bits from the second run; a lane that passed in a wave that runs again gets the same bits twice. So the
// second run needs no per-lane select. A short sequence on an operand outside its range returns some number or a NaN, traps nothing, and is never used.
// A stage function is written once, over these site forms: SHORT = the short sequence, the guard ANDed into ok; otherwise "guard ? short : plain", the helper above.
template <bool SHORT> XD float xd_site_rcp ( float d, int guard, int& ok ) {
    if constexpr ( SHORT ) { ok &= guard; return xd_rcp_short ( d ); }
    else { if ( guard ) return xd_rcp_short ( d ); return 1.f / d; }
}
template <bool SHORT> XD float xd_site_div_rk ( float x, float d, float r, int& ok ) {
    if constexpr ( SHORT ) { ok &= xd_in_range ( x ); return xd_div_short ( x, d, r ); }
    else return div_exact_rk ( x, d, r );
}
// The length of a vector that is nearly a unit vector -- an interpolated shading normal, a direction sampled about a wall's normal (where the reference's
// unnormalised tangent frame happens to be orthonormal) -- is one of the few floats around 1, and 1 - 2^-24, whose
// significand is all ones, is among them: three lengths in ten of random unit vectors, one in fifteen of a wall's interpolated normals (profiles/shade_stages/ab.md). Behind xd_normalize3's guard that is the plain
// division's arm in some lane of nearly every wave. A stage takes the reciprocal of such a length by its closed form instead, and its guard leaves the significand
// test out. For d = 2^k ( 2 - 2^-23 ): 1 / d = 2^-(k+1) ( 1 + 2^-24 + 2^-48 + .. ), a hair above the midpoint of 2^-(k+1) and its upper neighbour, so
// RN ( 1 / d ) = 2^-(k+1) ( 1 + 2^-23 ): biased exponent 253 - E for d's E, significand 1 (normal whenever d is inside the guarded range). The quotients' theorem
// (xd_div_short) asks for a correctly rounded reciprocal and excludes no significand. All 242 such d inside the range against 1.f / d: exhaustive. The quotients by them rest on
// the theorem; the unit entry's stage 4 also holds 2^24 hashed numerators, no more than 2^20 below their denominator, to "/" -- a sample, not a proof.
XD float xd_rcp_all_ones ( float d ) { return __uint_as_float ( ( 0x7e800000u - ( __float_as_uint ( d ) & 0x7f800000u ) ) | 1u | ( __float_as_uint ( d ) & 0x80000000u ) ); }
XD float xd_rcp_short_any ( float d ) { return ( __float_as_uint ( d ) & 0x7fffffu ) == 0x7fffffu ? xd_rcp_all_ones ( d ) : xd_rcp_short ( d ); }
XD int xd_normalize3_any_ok ( float x, float y, float z, float l ) {
    return ( int ) ( l >= 0x1p-60f ) & ( int ) ( l <= 0x1p60f ) & xd_component_ok ( x ) & xd_component_ok ( y ) & xd_component_ok ( z );
}
template <bool SHORT> XD void xd_site_normalize3 ( float x, float y, float z, float l, float& qx, float& qy, float& qz, int& ok ) {
    if constexpr ( SHORT ) {
        ok &= xd_normalize3_any_ok ( x, y, z, l );
        const float r = xd_rcp_short_any ( l );
        qx = xd_div_short_pos ( x, l, r ); qy = xd_div_short_pos ( y, l, r ); qz = xd_div_short_pos ( z, l, r );
    } else xd_normalize3 ( x, y, z, l, qx, qy, qz );
}
// Range tests that a stage's data cannot fail are not made there (DROPS in the stage functions; -DTERRA_SHADE_DROPS=0 keeps them all). The arguments:
//  * the reciprocal of a clamped density, rcp_exact ( sel_max ( pdf, 1e-4f ) ): sel_max is "pdf > 1e-4f ? pdf : 1e-4f", so the operand is >= 1e-4f > 2^-60 and never a
//    NaN (a NaN loses the comparison and the clamp returns 1e-4f). Only the upper bound and the significand test of xd_rcp_ok remain: xd_rcp_clamped_ok.
//  * a component of the next ray's direction (trace_math.h ray_stage): xd_rcp_unit_ok, the lower bound (which a NaN fails) and the significand test, no upper
//    bound. A camera direction is a normalised film vector rotated by a frame whose entries the host has checked to be at most 2 in magnitude (dev_types.h
//    terra_camera_stage_limits): below 8. A continuation direction is a quotient c / l of a component by its vector's length, at most 1 + 2^-21 in magnitude
//    whenever l > 0 (a denormal squared length has fewer bits, its root is still within a factor 1.5; l = inf gives 0 or a NaN). What is left is an infinity,
//    from l = 0 beside a non-zero component: a vector shorter than 2^-75. The continuation's vector is the tangent frame applied to
//    ( r cos, sqrt ( 1 - e ), r sin ) with sqrt ( 1 - e ) >= 2^-12, so along a normal n of roughly unit length it is at least 2^-13 long; and a normal that is
//    NOT of roughly unit length came from a length of 0 or infinity, has zeros, infinities or NaNs for components, and puts a product 0 * inf or a difference
//    inf - inf into every row of the frame: the vector is all NaN, or exactly zero (then 0 / 0), never tiny. tests/test_shade_stages_gpu.py holds that on
//    degenerate normals: no direction the guarded continuation returns has an infinite component.
XD int xd_rcp_unit_ok ( float d ) { return ( int ) ( __builtin_fabsf ( d ) >= 0x1p-60f ) & ( int ) ( ( __float_as_uint ( d ) & 0x7fffffu ) != 0x7fffffu ); }
XD int xd_rcp_clamped_ok ( float d ) { return ( int ) ( d <= 0x1p60f ) & ( int ) ( ( __float_as_uint ( d ) & 0x7fffffu ) != 0x7fffffu ); }
