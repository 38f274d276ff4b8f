// tdm_azimuth24 (csrc/dev_math.h) against tdm_sincosf_pair on every stream-B variate: both outputs as bit patterns, the quadrant formula against the reference
// reduction, and the early result's range against the reference's test -- all 2^24 arguments. Prints the first mismatch of each kind and the three counts;
// exit status 0 only when all are 0. Built and run by tests/test_azimuth24.py (host compiler, -ffp-contract=off as the library is built).
#include <stdio.h>
#include <stdint.h>
#include "dev_math.h"
#include "rng.h"

int main() {
    unsigned long long bad = 0, bad_quadrant = 0, bad_small = 0;
    for ( uint32_t k = 0; k < ( 1u << 24 ); ++k ) {
        const float y = TDM_AZIMUTH_SCALE * trng_b_from_bits ( k );
        float s0, c0, s1, c1;
        tdm_sincosf_pair ( y, s0, c0 );
        tdm_azimuth24 ( k, s1, c1 );
        if ( tdm_bits ( s0 ) != tdm_bits ( s1 ) || tdm_bits ( c0 ) != tdm_bits ( c1 ) ) {
            if ( !bad ) printf ( "first mismatch: k = %u, y = %a: tdm_sincosf_pair (%a, %a), tdm_azimuth24 (%a, %a)\n", k, y, s0, c0, s1, c1 );
            ++bad;
        }
        // the reference reduction (tdm_sincosf_pair): n = 0 in the unreduced arm
        int n = 0;
        if ( tdm_top12 ( y ) >= tdm_top12 ( 0x1.921FB6p-1f ) ) { const double r = ( double ) y * 0x1.45F306DC9C883p+23; n = ( ( int32_t ) r + 0x800000 ) >> 24; }
        if ( ( uint32_t ) n != tdm_azimuth24_quadrant ( k ) ) {
            if ( !bad_quadrant ) printf ( "first quadrant mismatch: k = %u: reference %d, tdm_azimuth24_quadrant %u\n", k, n, tdm_azimuth24_quadrant ( k ) );
            ++bad_quadrant;
        }
        if ( ( tdm_top12 ( y ) < tdm_top12 ( 0x1p-12f ) ) != ( k < 652u ) ) {
            if ( !bad_small ) printf ( "first early-result mismatch: k = %u, y = %a\n", k, y );
            ++bad_small;
        }
    }
    printf ( "mismatches %llu quadrant %llu early %llu\n", bad, bad_quadrant, bad_small );
    return ( bad || bad_quadrant || bad_small ) ? 1 : 0;
}
