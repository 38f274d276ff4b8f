// exact_sqrt.h -- correctly rounded float square roots in fewer instructions than the expansion of sqrtf (DESIGN.md 5 "Where the arithmetic legitimately differs",
// entry 5: the argument). sqrt_exact returns the bits sqrtf returns, for every input: inside a guarded range it takes the short sequence below, outside it it IS the
// plain sqrtf, behind a branch.
// Why the bits are sqrtf's. Under -fhip-fp32-correctly-rounded-divide-sqrt the compiler expands sqrtf ( x ) into 17 instructions in three parts:
//   scale-up     x < 2^-96 ? x 2^32 : x                                                    (v_mul, v_cmp, v_cndmask)
//   core         s = v_sqrt_f32 ( x ); the two neighbours of s, one unit of the last place down and up, formed on the integer pattern; the residuals x - s_down s and
//                x - s_up s, one fma each; s_down where the first is <= 0, then s_up where the second is > 0      (v_sqrt, 2 v_add_u32, 2 v_fma, 2 v_cmp, 2 v_cndmask)
//   epilogue     scaled ? s 2^-16 : s; x if x is +-0 or +inf                                (v_mul, v_cndmask, v_cmp_class, v_cndmask, a constant move)
// For a finite x >= 2^-96 the scale selects and the class select pass their first operand through. xs_sqrt_short is the core alone: the compiler's operations in the
// compiler's order on the same operand, so its result is the expansion's, bit for bit, by construction -- no rounding argument of this file's own is involved.
// The proof of record is the exhaustive comparison (tests/test_exact_sqrt_gpu.py: all 2^32 patterns against sqrtf). The claim is about THIS compiler's expansion:
// after a compiler upgrade read the expansion again (compile a one-line sqrtf kernel with the build's flags) and run that test.
// The A/B, site by site: profiles/short_sqrt/ab.md.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "exact_div.h"

XD float xs_sqrt_short ( float x ) {
    const float s = __builtin_amdgcn_sqrtf ( x );
    const float down = __uint_as_float ( __float_as_uint ( s ) - 1u ), up = __uint_as_float ( __float_as_uint ( s ) + 1u );
    const float r_down = __builtin_fmaf ( -down, s, x ), r_up = __builtin_fmaf ( -up, s, x );
    float r = r_down <= 0.f ? down : s;
    r = r_up > 0.f ? up : r;
    return r;
}
// the guarded range: finite and no smaller than 2^-96, the threshold of the expansion's scale-up (a NaN fails the first comparison, a negative value too). Ints joined
// with "&", as xd_in_range
XD int xs_in_range ( float x ) { return ( int ) ( x >= 0x1p-96f ) & ( int ) ( x <= 0x1.fffffep127f ); }
XD float sqrt_exact ( float x ) {
    if ( xs_in_range ( x ) ) return xs_sqrt_short ( x );
    return sqrtf ( x );
}
// the root as a site of a shading stage (exact_div.h "Shading stages"): SHORT = the short sequence, the guard ANDed into ok; otherwise sqrt_exact with that guard
template <bool SHORT> XD float xs_site_sqrt ( float x, int guard, int& ok ) {
    if constexpr ( SHORT ) { ok &= guard; return xs_sqrt_short ( x ); }
    else { if ( guard ) return xs_sqrt_short ( x ); return sqrtf ( x ); }
}
// Roots of a stream-B variate e = k 2^-24, k < 2^24 (rng.h trng_b_from_bits), whose range tests the data cannot fail (the stages' DROPS):
//  * sqrt ( e ): e is 0 or lies in [2^-24, 1 - 2^-24], far inside the guarded range: the guard is k != 0, one comparison (xs_variate_ok);
//  * sqrt ( sel_max ( 0, 1 - e ) ): 1 - e is exact and lies in [2^-24, 1]: no test at all.
// Both roots on all 2^24 variates against sqrt_exact: tests/test_shade_stages_gpu.py.
XD int xs_variate_ok ( float e ) { return ( int ) ( e != 0.f ); }
