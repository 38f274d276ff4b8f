// shading_device.h -- from a closest hit to a shaded surface (trace_device.h lists the layers): textures, the environment lookup,
// surface set-up, the raycast entry points, the BSDF presets and their dispatch.
#pragma once
#include "traverse_fast.h"

// -----------------------------------------------------------------------------
// textures (reference src/Terra.c:368-466; the rules where the reference is undefined: DESIGN.md 2a).
// uv is in TEXEL units, as the reference uses it ((size_t)uv->x). A texel is `components` elements;
// three consecutive elements are read from its first whatever `components` says, as the reference
// does: a 1- or 2-component texel returns its successors' elements too, a 4-component one drops its
// fourth, and past the last element of the data the section's two padding elements read as 0.
// A coordinate is used as it is inside (-1, 2^32): truncated towards zero to the texel, the bilinear
// weight u - texel (negative inside (-1, 0), as in the reference); u <= -1 and NaN count as 0,
// u >= 2^32 as the largest float below it (texture_coord). Mirror addressing takes the tile's parity
// from x alone and clamps the column W / row H it reaches at x % W == 0 / y % H == 0 to the last one.
// -----------------------------------------------------------------------------
TD float texture_coord ( float u ) { return u > -1.f ? fminf ( u, 4294967040.f ) : 0.f; }
TD V3 texture_read ( const DevTexture& t, uint32_t x, uint32_t y ) {
    const uint32_t W = t.width, H = t.height;
    if ( t.address_mode == 2 ) { x = x < W - 1 ? x : W - 1; y = y < H - 1 ? y : H - 1; }
    else if ( t.address_mode == 0 ) { x %= W; y %= H; }
    else if ( ( x / W ) % 2 == 0 ) { x %= W; y %= H; }
    else { x = W - ( x % W ); y = H - ( y % H ); x = x < W - 1 ? x : W - 1; y = y < H - 1 ? y : H - 1; }
    const size_t e = ( ( size_t ) y * W + x ) * t.components;
    if ( t.depth == 1 ) {
        const uint8_t* p = reinterpret_cast<const uint8_t*> ( t.data ) + e;
        return v3 ( p[0] / 255.f, p[1] / 255.f, p[2] / 255.f );
    }
    const float* p = reinterpret_cast<const float*> ( t.data ) + e;
    return v3 ( p[0], p[1], p[2] );
}
TD V3 texture_sample ( const DevTexture& t, float u, float v ) {
    u = texture_coord ( u ); v = texture_coord ( v );
    uint32_t ix = ( uint32_t ) u, iy = ( uint32_t ) v;
    if ( t.filter == 0 ) return texture_read ( t, ix, iy );
    if ( t.filter != 1 ) return v3 ( 0, 0, 0 );          // trilinear / anisotropic: unimplemented in the reference too (returns zero)
    uint32_t x2 = ix + 1 < t.width - 1 ? ix + 1 : t.width - 1, y2 = iy + 1 < t.height - 1 ? iy + 1 : t.height - 1;
    V3 n1 = texture_read ( t, ix, iy ), n2 = texture_read ( t, x2, iy ), n3 = texture_read ( t, ix, y2 ), n4 = texture_read ( t, x2, y2 );
    float wu = u - ( float ) ix, wv = v - ( float ) iy, wou = 1.f - wu, wov = 1.f - wv;
    return v3 ( ( n1.x * wou + n2.x * wu ) * wov + ( n3.x * wou + n4.x * wu ) * wv,
                ( n1.y * wou + n2.y * wu ) * wov + ( n3.y * wou + n4.y * wu ) * wv,
                ( n1.z * wou + n2.z * wu ) * wov + ( n3.z * wou + n4.z * wu ) * wv );
}

#define TERRA_PI_F 3.1416926535f        // the reference's terra_PI (include/TerraMath.h), not pi
#define TERRA_INV_PI_F 0x1.45f06p-2f    // 1.f / TERRA_PI_F, correctly rounded (0.3182997703552246), for div_exact_rk
static_assert ( TERRA_INV_PI_F == 1.f / TERRA_PI_F, "the literal is the compiler's own correctly rounded quotient" );
// lat-long environment lookup by direction (reference src/Terra.c:468-477): nearest texel, no filtering.
// terra_PI exceeds pi, so phi / (2 terra_PI) and theta / terra_PI stay below 1 and the texel is in range.
TD V3 environment_eval ( const DevScene& sc, V3 dir ) {
    if ( sc.env_mode == 1 ) return v3 ( sc.env_color[0], sc.env_color[1], sc.env_color[2] );
    const DevTexture& t = sc.textures[sc.env_tex];
    V3 d = normalize ( dir );
    float theta = tdm_acosf ( d.y );
    float phi = tdm_atan2f ( d.z, d.x ) + TERRA_PI_F;
    uint32_t u = ( uint32_t ) texture_coord ( ( phi / ( 2 * TERRA_PI_F ) ) * ( float ) t.width );      // (a direction without a length gives NaN: texel 0)
    uint32_t v = ( uint32_t ) texture_coord ( ( theta / TERRA_PI_F ) * ( float ) t.height );
    return texture_read ( t, u, v );
}

// -----------------------------------------------------------------------------
// surface
// -----------------------------------------------------------------------------
// The reference also stores the tangent frame (terra_f4x4_basis of the normal) in the
// surface; it is a pure function of the normal, so it is rebuilt where it is consumed
// (diffuse sampling) instead of being carried in 9 registers.
struct Surface {
    V3    normal;
    V3    emissive;
    V3    attr[4];      // the presets use at most 4 slots; Phong slot 3.x and glass slots 2, 3.x are scratch written by sample()
    float ior;
    int   bsdf;
};

// Stage S2 of the shading stages (exact_div.h "Shading stages"): the hit's barycentrics from the triangle's staged constants (div2_exact with the denominator's
// part done ahead: flag stands for xd_rcp_ok ( div ), rdiv for xd_rcp_short ( div )) and the interpolated normal's normalisation -- three sites. Returns the lane's
// mask. SHORT = false: surface_init's own lines. No range test is left out here: a hit on an edge has nu == 0, a cancelled normal component can be arbitrarily small.
template <bool SHORT> TD int surface_stage ( float nu, float nv, float div, float rdiv, int flag, V3 na, V3 nb, V3 nc, float& u, float& v, V3& normal ) {
    int ok = 1;
    const int g = flag & xd_in_range ( nu ) & xd_in_range ( nv );
    if constexpr ( SHORT ) ok &= g;
    if ( SHORT || g ) { u = xd_div_short ( nu, div, rdiv ); v = xd_div_short ( nv, div, rdiv ); }
    else { u = nu / div; v = nv / div; }
    const float w = 1 - u - v;
    normal = normalize_site<SHORT> ( ( nc * v + nb * u ) + na * w, ok );
    return ok;
}
// STAGED (the kernels of ray_start_masks_for, pair-form launches): u, v and the normal by surface_stage, one vote
template <int MODE, int KINDS, bool STAGED = false>
TD void surface_init ( const Tracer& T, uint32_t ti, V3 point, Surface& sf, uint32_t& object_out, uint32_t& tri_in_object_out, uint32_t& nattr_out ) {
    float4 t0, t1, t2, p0, p1, p2, p3x;
    if ( MODE == 1 ) {
        const float4* lt = reinterpret_cast<const float4*> ( T.l_tris );
        t0 = lt[3 * ti]; t1 = lt[3 * ti + 1]; t2 = lt[3 * ti + 2];
        p0 = T.l_props[4 * ti]; p1 = T.l_props[4 * ti + 1]; p2 = T.l_props[4 * ti + 2]; p3x = T.l_props[4 * ti + 3];
    } else {
        const float4* tris = reinterpret_cast<const float4*> ( MODE >= 2 ? T.sc.fast_tris : T.sc.tris );
        const float4* props = reinterpret_cast<const float4*> ( T.sc.props );
        t0 = tris[3 * ti]; t1 = tris[3 * ti + 1]; t2 = tris[3 * ti + 2];
        uint32_t pi = ti;
        if ( MODE >= 2 ) pi = T.sc.mats[__float_as_uint ( t0.w )].first_tri + __float_as_uint ( t1.w );
        p0 = props[4 * pi]; p1 = props[4 * pi + 1]; p2 = props[4 * pi + 2]; p3x = props[4 * pi + 3];
    }
    uint32_t object = __float_as_uint ( t0.w );
    object_out = object; tri_in_object_out = __float_as_uint ( t1.w );
    float u, v;
    if ( MODE == 1 && T.l_consts ) {          // pair-form launches: e0, e1, d00, d11, d01, div as make_tracer formed them once per block, by these very operations
        const float4 c0 = T.l_consts[3 * ti], c1 = T.l_consts[3 * ti + 1], c2 = T.l_consts[3 * ti + 2];
        const V3 e0 = v3 ( c0.x, c0.y, c0.z ), e1 = v3 ( c0.w, c1.x, c1.y ), p = point - v3 ( t0.x, t0.y, t0.z );
        const float d00 = c1.z, d11 = c1.w, d01 = c2.x, div = c2.y;
        const float dp0 = dot ( p, e0 ), dp1 = dot ( p, e1 );
        const float nu = d11 * dp0 - d01 * dp1, nv = d00 * dp1 - d01 * dp0;
        // the flag word stands for xd_rcp_ok ( div ), c2.z for xd_rcp_short ( div ): div2_exact with its denominator's part done ahead
        if constexpr ( STAGED ) {
            const V3 na = v3 ( p0.x, p0.y, p0.z ), nb = v3 ( p0.w, p1.x, p1.y ), nc = v3 ( p1.z, p1.w, p2.x );
            if ( __any ( !surface_stage<true> ( nu, nv, div, c2.z, ( int ) __float_as_uint ( c2.w ), na, nb, nc, u, v, sf.normal ) ) )
                surface_stage<false> ( nu, nv, div, c2.z, ( int ) __float_as_uint ( c2.w ), na, nb, nc, u, v, sf.normal );
        } else
        if ( ( int ) __float_as_uint ( c2.w ) & xd_in_range ( nu ) & xd_in_range ( nv ) ) { u = xd_div_short ( nu, div, c2.z ); v = xd_div_short ( nv, div, c2.z ); }
        else { u = nu / div; v = nv / div; }
    } else {
        V3 ta, tb, tc; tri_vertices ( t0, t1, t2, ta, tb, tc );
        V3 e0 = tb - ta, e1 = tc - ta, p = point - ta;
        float d00 = dot ( e0, e0 ), d11 = dot ( e1, e1 ), d01 = dot ( e0, e1 );
        float dp0 = dot ( p, e0 ), dp1 = dot ( p, e1 );
        float div = d00 * d11 - d01 * d01;
        div2_exact ( d11 * dp0 - d01 * dp1, d00 * dp1 - d01 * dp0, div, u, v );
    }
    float w = 1 - u - v;
    V3 na = v3 ( p0.x, p0.y, p0.z ), nb = v3 ( p0.w, p1.x, p1.y ), nc = v3 ( p1.z, p1.w, p2.x );
    if ( !STAGED || ! ( MODE == 1 && T.l_consts ) ) sf.normal = normalize ( ( nc * v + nb * u ) + na * w );          // (STAGED: the pair-form branch above has made it)
    const DevMaterial& m = T.l_mats[object];
    sf.emissive = v3p ( m.emissive );
    #pragma unroll
    for ( int i = 0; i < 4; ++i ) sf.attr[i] = v3p ( m.attributes[i] );
    if ( ( KINDS & TERRA_KIND_TEX ) && m.any_texture ) {       // textured attributes: interpolate the texcoord as the reference does (src/Terra.c:1748-1752) and sample
        V3 pa2 = v3 ( p2.y, p2.z, 0.f );            // texcoord_a
        V3 pb2 = v3 ( p2.w, p3x.x, 0.f );           // texcoord_b
        V3 pc2 = v3 ( p3x.y, p3x.z, 0.f );          // texcoord_c
        float tx = ( pc2.x * v + pb2.x * u ) + pa2.x * w;
        float ty = ( pc2.y * v + pb2.y * u ) + pa2.y * w;
        #pragma unroll
        for ( int i = 0; i < 4; ++i ) if ( m.tex[i] >= 0 ) sf.attr[i] = texture_sample ( T.sc.textures[m.tex[i]], tx, ty );
        if ( m.tex[TERRA_DEV_MAX_ATTR] >= 0 ) sf.emissive = texture_sample ( T.sc.textures[m.tex[TERRA_DEV_MAX_ATTR]], tx, ty );
    }
    sf.bsdf = m.bsdf;
    sf.ior = m.ior;
    nattr_out = m.attributes_count;
}

struct RaycastResult { bool hit; uint32_t object, tri_in_object, tri; V3 point; };

struct Azimuth { float sn, cs; uint32_t k; int kind; };
struct PathDraws { float e0, e1, e2, e3; Azimuth az; };
// the azimuth table a kernel of tree mode MODE may read: only LDS-resident launches are ever handed one (scene_host.cpp fill_params), so every other instance
// is compiled without the load and its branch
template <int MODE> TD const float2* azimuth_table ( const DevScene& sc ) { return MODE == 1 ? sc.sincos24 : nullptr; }
template <int COUNT> TD PathDraws path_draw ( const float2* sincos24, Pcg32& rb, Counters& c );

// guarded (the kernels of ray_start_masks_for): what make_ray_guarded found for this lane's ray
// pre / rb (optional): a hit draws the path's four continuation variates (path_draw) BEFORE the surface is set up, so that the azimuth table load they issue
// is in flight during terra_surface_init's arithmetic -- only for integrators that draw nothing of their own between the hit and the BSDF sample
template <int COUNT, int MODE, int KINDS>
TD RaycastResult scene_raycast ( const Tracer& T, const Ray& in, Surface& sf, Counters& c, PathDraws* pre = nullptr, Pcg32* rb = nullptr, bool guarded = false ) {
    Ray r = in;
    r.o = r.o + r.d * 0.001f;
    constexpr bool MASKS = ray_start_masks_for ( COUNT, MODE, KINDS );          // (trace_geometry.h: the ray start by lane predicates, one range test)
    if ( COUNT ) ++c.rays;
    Closest best;
    if constexpr ( MASKS ) { V3 o_perm; const RayStateMasks st = ray_start_masks ( r, o_perm ); best = bvh_traverse_from<COUNT, MODE> ( T, r, st, o_perm, c, __all ( guarded ) != 0 ); }
    else {
    RayState st = ray_state_init ( r );
    if ( MODE >= 2 ) { ClosestRanked b2 = bvh_traverse_fast<COUNT, MODE == 3> ( T, r, st, c ); best.depth = b2.depth; best.tri = b2.tri; }
    else best = bvh_traverse<COUNT, MODE> ( T, r, st, c );
    }
    RaycastResult res; res.hit = best.tri != 0xffffffffu; res.tri = best.tri; res.object = 0; res.tri_in_object = 0;
    res.point = res.hit ? r.o + r.d * best.depth : v3 ( FLT_MAX, FLT_MAX, FLT_MAX );
    if ( res.hit ) {
        uint32_t nattr;
        if ( pre ) *pre = path_draw<COUNT> ( azimuth_table<MODE> ( T.sc ), *rb, c );
        surface_init<MODE, KINDS, MASKS && TERRA_SHADE_STAGES != 0> ( T, best.tri, res.point, sf, res.object, res.tri_in_object, nattr );
        if ( MODE >= 2 ) res.tri = T.sc.mats[res.object].first_tri + res.tri_in_object;      // back to the soup index (lights, areas)
        if ( COUNT ) ++c.hits;
        if ( COUNT == 2 ) c.attr_fetches += nattr + 1;
    }
    return res;
}

// terra_scene_raycast for a ray of which only "which triangle is hit first" matters (the shadow ray of the Direct integrator, src/Terra.c:1349-1426, on scenes whose
// emissive attributes are constants): same traversal, same counts -- a hit is a surface initialisation in the reference -- without setting the surface up.
// Returns the triangle's index in the soup (the index the light tables use), 0xffffffff for a miss.
// `expected` (soup index): the only answer the caller distinguishes from the others; kernels without counters then take the shortcut of fast_expect on MODE 2
// MASKS: ray_start_masks_for of the calling kernel (only its MODE 1, COUNT 0 block looks at it)
template <int COUNT, int MODE, bool MASKS = false>
TD uint32_t scene_raycast_triangle ( const Tracer& T, const Ray& in, Counters& c, uint32_t expected ) {
    Ray r = in;
    r.o = r.o + r.d * 0.001f;
    V3 o_masks = v3 ( 0, 0, 0 );
    const auto st = [&] { if constexpr ( MASKS ) return ray_start_masks ( r, o_masks ); else return ray_state_init ( r ); } ();
    if ( COUNT ) ++c.rays;
    if constexpr ( MODE == 2 && COUNT == 0 ) {
        const V3 o_perm = permuted ( r.o, st );
        ClosestRanked best;
        if ( !fast_expect ( T, st, o_perm, expected, best ) ) return 0xffffffffu;          // (not the expected triangle; without counters nothing else is asked)
        int* top = T.stack; uint32_t hand = TERRA_FAST_ROOT_IN_HAND, held = 0u;
        traverse_fast_resume<COUNT> ( T, r, st, o_perm, best, top, hand, held, 0, c, false, true );
        return best.tri == TERRA_TRI_EXPECTED ? expected : 0xffffffffu;
    }
    // LDS-resident scenes, every tree mode: the reference's traversal order is kept, so "comes first" is its own strict "<" -- with the closest hit preset to ONE ULP
    // BEYOND the expected triangle's depth, a triangle as near as the expected one wins exactly when the reference meets it earlier; the expected triangle itself, when
    // its leaf is reached, takes the record as it would; and the traversal ends at the first OTHER triangle that takes it (traverse_loops ANYHIT): up to there it has
    // made the reference's decisions one by one, after that none can change the answer. A ray that misses its triangle is not traced at all.
    if constexpr ( MODE == 1 && COUNT == 0 ) {
        const V3 o_perm = MASKS ? o_masks : permuted ( r.o, st );
        float depth;
        if ( !watertight_permuted ( tri_perm_lds ( T.l_tris + 12 * expected, st ), o_perm, st, depth ) ) return 0xffffffffu;
        Closest best; best.depth = __uint_as_float ( __float_as_uint ( depth + 0.f ) + 1u ); best.tri = 0xffffffffu;      // (depth >= 0; + 0.f: -0 -> +0)
        // pair form (traverse_ref.h traverse_pairs): the trips are not in rank order, so the record is preset to the expected triangle's own (depth, key) exactly and the
        // first triangle that beats it in that order answers "another one" (key 0)
        if ( T.pairs ) { best.depth = depth; best.tri = terra_pair_key ( __float_as_uint ( T.l_tris[12 * expected + 11] ), expected ); }
        if ( T.fused && __all ( ray_is_tame ( r ) ) ) traverse_loops<COUNT, MODE, true, true, true> ( T, r, st, o_perm, best, c, expected );
        else if ( __all ( ray_is_regular ( r ) ) ) traverse_loops<COUNT, MODE, true, false, true> ( T, r, st, o_perm, best, c, expected );
        else traverse_loops<COUNT, MODE, false, false, true> ( T, r, st, o_perm, best, c, expected );
        if ( T.pairs ) return best.tri != 0u ? expected : 0xffffffffu;
        return best.tri;
    }
    uint32_t tri;
    if ( MODE >= 2 ) { const ClosestRanked b2 = bvh_traverse_fast<COUNT, MODE == 3> ( T, r, st, c ); tri = b2.tri; }
    else tri = bvh_traverse<COUNT, MODE> ( T, r, st, c ).tri;
    if ( tri == 0xffffffffu ) return tri;
    uint32_t object;
    if ( MODE == 1 ) object = __float_as_uint ( T.l_tris[12 * tri + 3] );
    else {
        const float4* tris = reinterpret_cast<const float4*> ( MODE >= 2 ? T.sc.fast_tris : T.sc.tris );
        const float4 t0 = tris[3 * tri];
        object = __float_as_uint ( t0.w );
        if ( MODE >= 2 ) tri = T.sc.mats[object].first_tri + __float_as_uint ( tris[3 * tri + 1].w );      // back to the soup index
    }
    if ( COUNT ) ++c.hits;
    if ( COUNT == 2 ) c.attr_fetches += T.l_mats[object].attributes_count + 1;
    return tri;
}

// where a ray that leaves the surface at p starts: off it along the shading normal (terra_surface_ray, src/Terra.c:1715, with sign +1: the only sign its callers pass).
// The render loops keep this origin and a direction and take the ray's reciprocals (make_ray) when the ray starts.
TD V3 surface_origin ( const Surface& sf, V3 p ) { return p + sf.normal * 0.0001f; }
TD Ray surface_ray ( const Surface& sf, V3 p, V3 d ) { return make_ray ( surface_origin ( sf, p ), d ); }

// -----------------------------------------------------------------------------
// BSDF presets
// -----------------------------------------------------------------------------

// sin / cos of the azimuth 2 * terra_PI * e that the samplers make of one variate (src/TerraPresets.c:39-40). A stream-B variate is u24 * 2^-24
// (rng.h), so over the render path this is a pure function of 24 bits, and it is had in one of two ways, same bits either way:
// * computed from the 24 bits by tdm_azimuth24 (dev_math.h: the glibc algorithm in one arm, the quadrant from the integer; ~45 instructions) -- the default;
// * read from DevScene::sincos24, which tabulates it -- every entry computed by tdm_sincosf_pair itself, when the first scene that asks for the table is
//   committed (unit_kernels.hip terra_fill_sincos24; terra_amd_set_azimuth_table) -- one 8-byte load of a uniformly random entry of 128 MB.
// Any other argument (unit-level calls with arbitrary variates, a sampler-driven first bounce) takes tdm_sincosf_pair.
// kind 0: nothing held (the sampler computes from its float); 1: (sn, cs) are the table's entry; 2: k holds the variate's 24 bits
static_assert ( TDM_AZIMUTH_SCALE == 2 * TERRA_PI_F, "tdm_azimuth24's scale is the samplers' 2 * terra_PI" );
TD Azimuth azimuth_none() { Azimuth a; a.sn = 0.f; a.cs = 1.f; a.k = 0u; a.kind = 0; return a; }
// the variate whose 24 bits the caller holds (path_draw, the integrators' own draws): the table's load is issued here and the caller uses it as late as it can
TD Azimuth azimuth_fetch_index ( const float2* tab, uint32_t k ) {
    Azimuth a = azimuth_none();
    if ( tab ) { const float2 v = tab[k]; a.cs = v.x; a.sn = v.y; a.kind = 1; }
    else { a.k = k; a.kind = 2; }
    return a;
}
// the same for a float: e is one of the 2^24 stream-B values exactly when e * 2^24 is a whole number below 2^24
TD Azimuth azimuth_fetch ( const float2* tab, float e ) {
    const float x = e * 16777216.f;
    if ( e >= 0.f && x < 16777216.f ) {
        const uint32_t k = ( uint32_t ) x;
        if ( ( float ) k == x ) return azimuth_fetch_index ( tab, k );
    }
    return azimuth_none();
}
TD void azimuth_sincos ( const Azimuth& az, float e, float& sn, float& cs ) {
    if ( az.kind == 1 ) { sn = az.sn; cs = az.cs; }
    else if ( az.kind == 2 ) tdm_azimuth24 ( az.k, sn, cs );
    else tdm_sincosf_pair ( 2 * TERRA_PI_F * e, sn, cs );
}

// (diffuse_sample, diffuse_pdf, diffuse_eval and path_continue<1> are restated, operation for operation, in integrators_device.h continue_stage for the kernels that
// shade in stages: a change of any of them goes into both. terra_amd_unit_shade_stages holds continue_stage to path_continue<1> itself, bit for bit.)
TD V3 diffuse_sample ( const Surface& sf, float e1, float e2, const Azimuth& az ) {
    float r = sqrt_exact ( e1 );
    float sn, cs;
    azimuth_sincos ( az, e2, sn, cs );
    float x = r * cs;
    float z = r * sn;
    V3 wi = v3 ( x, sqrt_exact ( sel_max ( 0.f, 1 - e1 ) ), z );
    return normalize ( basis_apply ( make_basis ( sf.normal ), wi ) );
}
TD float diffuse_pdf ( const Surface& sf, V3 wi ) { return div_exact_rk ( sel_max ( 0.f, dot ( sf.normal, wi ) ), TERRA_PI_F, TERRA_INV_PI_F ); }
TD V3 diffuse_eval ( const Surface& sf ) { return sf.attr[0] * ( float ) ( 1. / ( double ) TERRA_PI_F ); }

TD void phong_kd_ks ( const Surface& sf, float& kd, float& ks ) {
    V3 al = sf.attr[1], sp = sf.attr[0];
    float diffuse = sel_max ( al.x + al.y + al.z, ( float ) 1e-4 );
    float specular = sp.x + sp.y + sp.z;
    if ( specular > diffuse ) { kd = 0.5f * diffuse / specular; ks = 1.f - kd; }
    else { ks = 0.5f * specular / diffuse; kd = 1.f - ks; }
}
TD V3 phong_reflect ( const Surface& sf, V3 wo ) { return sf.normal * ( 2.f * dot ( wo, sf.normal ) ) - wo; }

TD V3 phong_sample ( Surface& sf, float e1, float e2, float e3, V3 wo, const Azimuth& az ) {
    float kd, ks; phong_kd_ks ( sf, kd, ks );
    if ( e3 < kd ) { sf.attr[3].x = 1.f; return diffuse_sample ( sf, e1, e2, az ); }
    sf.attr[3].x = -1.f;
    V3 wr = phong_reflect ( sf, wo );
    Basis b = make_basis ( wr );
    float phi = 2 * TERRA_PI_F * e1;
    float theta = tdm_acosf ( tdm_powf ( 1.f - e2, 1.f / ( sf.attr[2].x + 1 ) ) );
    float sin_theta = tdm_sinf ( theta );
    V3 wi = v3 ( sin_theta * tdm_cosf ( phi ), tdm_cosf ( theta ), sin_theta * tdm_sinf ( phi ) );
    return normalize ( basis_apply ( b, wi ) );
}
TD float phong_pdf ( const Surface& sf, V3 wi, V3 wo ) {
    if ( sf.attr[3].x == 1.f ) return diffuse_pdf ( sf, wi );
    V3 wr = phong_reflect ( sf, wo );
    float cos_alpha = dot ( wi, wr );
    float n = sf.attr[2].x;
    return ( n + 1 ) / ( 2 * TERRA_PI_F ) * tdm_powf ( cos_alpha, n );
}
TD V3 phong_eval ( const Surface& sf, V3 wi, V3 wo ) {
    float kd, ks; phong_kd_ks ( sf, kd, ks );
    float n = sf.attr[2].x;
    V3 diffuse_term = sf.attr[1] * ( kd * 1.f / TERRA_PI_F );
    V3 wr = phong_reflect ( sf, wo );
    float cos_alpha = dot ( wi, wr );
    float cos_n_alpha = tdm_powf ( cos_alpha, n );
    V3 specular_term = sf.attr[0] * ( ks * cos_n_alpha * ( n + 2 ) / ( 2 * TERRA_PI_F ) );
    return diffuse_term + specular_term;
}

// ---- GGX conductor and dielectric glass: defined by this repo (include/TerraPresets.h), no live
// reference; building blocks from the reference's dead code (src/TerraPresets.c:303-320, 333-343, 399-449)
TD float ggx_D ( float NoH, float alpha2 ) {
    if ( NoH <= 0.f ) return 0.f;
    float NoH2 = NoH * NoH;
    float den = NoH2 * alpha2 + ( 1 - NoH2 );
    return alpha2 / ( TERRA_PI_F * den * den );
}
TD float ggx_G1 ( V3 v, V3 n, V3 h, float alpha2 ) {
    float VoH = dot ( v, h ), VoN = dot ( v, n );
    if ( VoH / VoN <= 0.f ) return 0.f;
    float VoN2 = VoN * VoN;
    float tan2 = ( 1.f - VoN2 ) / VoN2;        // Smith G1 w.r.t. the normal (Walter 2007 eq. 34), see oracle note
    return 2.f / ( sqrt_exact ( 1 + alpha2 * tan2 ) + 1 );
}
TD V3 ggx_sample ( const Surface& sf, float e1, float e2, V3 wo, const Azimuth& az ) {
    float alpha = sf.attr[1].x;
    float t2 = alpha * alpha * e1 / ( 1.f - e1 );
    float cos_t = 1.f / sqrt_exact ( 1.f + t2 );
    float sin_t = sqrt_exact ( t2 ) * cos_t;            // tan * cos: sqrt ( 1 - cos_t^2 ) cancels (absolute error ~2^-11.5 whatever alpha)
    float sn, cs;
    azimuth_sincos ( az, e2, sn, cs );
    V3 h = v3 ( sin_t * cs, cos_t, sin_t * sn );
    h = normalize ( basis_apply ( make_basis ( sf.normal ), h ) );
    float HoV = sel_max ( 0.f, dot ( h, wo ) );
    return h * ( 2 * HoV ) - wo;
}
TD float ggx_pdf ( const Surface& sf, V3 wi, V3 wo ) {
    float alpha = sf.attr[1].x;
    V3 h = normalize ( wi + wo );
    float NoH = dot ( sf.normal, h ), HoV = dot ( h, wo );
    if ( ! ( HoV > 0.f ) ) return 0.f;                  // wi = -wo (the sampler's clamp) makes h = normalize ( 0 ) = NaN: NaN takes this branch
    return ggx_D ( NoH, alpha * alpha ) * NoH / ( 4.f * HoV );
}
TD V3 ggx_eval ( const Surface& sf, V3 wi, V3 wo ) {
    float alpha = sf.attr[1].x, alpha2 = alpha * alpha;
    float NoL = dot ( sf.normal, wi ), NoV = dot ( sf.normal, wo );
    if ( NoL <= 0.f || NoV <= 0.f ) return v3 ( 0, 0, 0 );
    V3 h = normalize ( wi + wo );
    float NoH = dot ( sf.normal, h ), HoV = sel_max ( 0.f, dot ( h, wo ) );
    float m = sel_max ( 0.f, 1.f - HoV ), m2 = m * m, w5 = m2 * m2 * m;            // h.wo can round above 1 (wo = n = wi): no negative Schlick weight
    V3 F0 = sf.attr[0];
    V3 F = v3 ( F0.x + ( 1.f - F0.x ) * w5, F0.y + ( 1.f - F0.y ) * w5, F0.z + ( 1.f - F0.z ) * w5 );
    float G = ggx_G1 ( wo, sf.normal, h, alpha2 ) * ggx_G1 ( wi, sf.normal, h, alpha2 );
    float k = G * ggx_D ( NoH, alpha2 ) / ( 4.f * NoL * NoV );
    return F * k;
}
TD V3 glass_sample ( Surface& sf, float e3, V3 wo ) {
    V3 normal = sf.normal, incident = neg ( wo );
    float n1, n2, cos_i = dot ( normal, incident );
    if ( cos_i > 0.f ) { n1 = sf.ior; n2 = 1.f; normal = neg ( normal ); }
    else { n1 = 1.f; n2 = sf.ior; cos_i = -cos_i; }
    V3 refl = incident - normal * ( 2 * dot ( normal, incident ) );
    float nni = n1 / n2;
    float nni2 = nni * nni;
    float cos_t2 = ( 1.f - nni2 ) + nni2 * ( cos_i * cos_i );      // = 1 - nni^2 ( 1 - cos_i^2 ) without rounding 1 - cos_i^2 to 1 at grazing incidence (ior 1: exactly cos_i^2)
    V3 dir; float prob;
    if ( cos_t2 < 0.f ) { dir = refl; prob = 1.f; }
    else {
        float cos_t = sqrt_exact ( cos_t2 );
        float t = 1.f - ( n1 <= n2 ? cos_i : cos_t );
        float R0 = ( n1 - n2 ) / ( n1 + n2 ); R0 *= R0;
        float R = R0 + ( 1 - R0 ) * ( t * t * t * t * t );
        if ( e3 < R ) { dir = refl; prob = R; }
        else {
            V3 tv = normal * ( nni * cos_i - cos_t ), tn = incident * nni;
            dir = normalize ( tv + tn ); prob = 1 - R;
        }
    }
    sf.attr[2] = dir; sf.attr[3].x = prob;
    return dir;
}
TD bool glass_is_sampled ( const Surface& sf, V3 wi ) {
    return sf.attr[3].x > 0.f && wi.x == sf.attr[2].x && wi.y == sf.attr[2].y && wi.z == sf.attr[2].z;
}
TD float glass_pdf ( const Surface& sf, V3 wi ) { return glass_is_sampled ( sf, wi ) ? sf.attr[3].x : 0.f; }
TD V3 glass_eval ( const Surface& sf, V3 wi ) {
    if ( !glass_is_sampled ( sf, wi ) ) return v3 ( 0, 0, 0 );
    float c = dot ( sf.normal, wi );
    if ( c == 0.f ) return v3 ( 0, 0, 0 );         // a direction in the surface's plane (wo tangent; refraction at exactly the critical angle): the path dies, no inf * 0
    float k = sf.attr[3].x / c;
    return sf.attr[0] * k;
}

// BSDF dispatch. KINDS is a compile-time mask of the preset kinds present in the committed scene
// (bit k = DevBsdfKind k): a diffuse-only scene compiles to straight-line diffuse code, which is
// what keeps the Simple kernel inside 96 VGPRs (5 waves/SIMD) without scratch.
#define TERRA_KINDS_ALL 127
// az: the azimuth of the SECOND variate (e2), as azimuth_fetch / azimuth_fetch_index hold it -- what the diffuse and GGX samplers and Phong's diffuse branch use
template <int KINDS>
TD V3 bsdf_sample ( Surface& sf, float e1, float e2, float e3, V3 wo, const Azimuth& az ) {
    if ( ( KINDS & 2 ) && ( KINDS == 2 || sf.bsdf == kDevBsdfPhong ) ) return phong_sample ( sf, e1, e2, e3, wo, az );
    if ( ( KINDS & 4 ) && ( KINDS == 4 || sf.bsdf == kDevBsdfGGX ) ) return ggx_sample ( sf, e1, e2, wo, az );
    if ( ( KINDS & 8 ) && ( KINDS == 8 || sf.bsdf == kDevBsdfGlass ) ) return glass_sample ( sf, e3, wo );
    return diffuse_sample ( sf, e1, e2, az );
}
template <int KINDS>
TD float bsdf_pdf ( const Surface& sf, V3 wi, V3 wo ) {
    if ( ( KINDS & 2 ) && ( KINDS == 2 || sf.bsdf == kDevBsdfPhong ) ) return phong_pdf ( sf, wi, wo );
    if ( ( KINDS & 4 ) && ( KINDS == 4 || sf.bsdf == kDevBsdfGGX ) ) return ggx_pdf ( sf, wi, wo );
    if ( ( KINDS & 8 ) && ( KINDS == 8 || sf.bsdf == kDevBsdfGlass ) ) return glass_pdf ( sf, wi );
    return diffuse_pdf ( sf, wi );
}
template <int KINDS>
TD V3 bsdf_eval ( const Surface& sf, V3 wi, V3 wo ) {
    if ( ( KINDS & 2 ) && ( KINDS == 2 || sf.bsdf == kDevBsdfPhong ) ) return phong_eval ( sf, wi, wo );
    if ( ( KINDS & 4 ) && ( KINDS == 4 || sf.bsdf == kDevBsdfGGX ) ) return ggx_eval ( sf, wi, wo );
    if ( ( KINDS & 8 ) && ( KINDS == 8 || sf.bsdf == kDevBsdfGlass ) ) return glass_eval ( sf, wi );
    return diffuse_eval ( sf );
}
