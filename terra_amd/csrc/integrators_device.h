// integrators_device.h -- top layer of the device hot path (trace_device.h lists the layers): light and environment sampling, the
// integrators and their split forms, the path tail, the sampler pair, one full path, the tonemapper.
#pragma once
#include "shading_device.h"

// -----------------------------------------------------------------------------
// lights and integrators
// -----------------------------------------------------------------------------
// COUNT levels: 0 none (the default launch); 2 = rays, nodes, triangle tests, hits, stream-B draws, attribute fetches per lane
TD float randf ( Pcg32& b, Counters& c, int count ) { if ( count == 2 ) ++c.rand_calls; return trng_b_float ( b ); }
// the same draw as its 24 bits: randf = trng_b_from_bits ( randf_bits )
TD uint32_t randf_bits ( Pcg32& b, Counters& c, int count ) { if ( count == 2 ) ++c.rand_calls; return trng_b_bits ( b ); }

TD float triangle_area ( V3 a, V3 b, V3 cc ) { return length ( cross ( b - a, cc - a ) ) / 2; }

struct LightSample { uint32_t light_object; uint32_t tri_in_object; uint32_t tri; float pick_pdf; V3 pos, norm; };

// (MODE 1: the light's triangle and vertex normals come from the block's LDS copy of the scene)
template <int COUNT, int MODE = 0>
TD LightSample draw_light_sample ( const DevScene& sc, Pcg32& rb, Counters& c, const Tracer* T = nullptr ) {
    LightSample ls;
    float e = ( float ) ( ( double ) randf ( rb, c, COUNT ) - 1e-4 );
    double xl = ( double ) e * ( double ) sc.n_lights;
    uint32_t li = xl < 0 ? 0u : ( uint32_t ) xl;
    ls.pick_pdf = 1.f / ( float ) sc.lights_triangles_count;
    DevLight l = ( MODE == 1 && T ) ? T->l_lights[li] : sc.lights[li];
    float e_t = randf ( rb, c, COUNT );
    uint32_t k = ( uint32_t ) ( e_t * ( float ) l.tri_count );
    if ( k >= l.tri_count ) k = l.tri_count - 1;
    ls.light_object = l.object; ls.tri_in_object = k; ls.tri = l.first_tri + k;
    float e1 = randf ( rb, c, COUNT ), e2 = randf ( rb, c, COUNT );
    const float4* tris = ( MODE == 1 && T ) ? reinterpret_cast<const float4*> ( T->l_tris ) : reinterpret_cast<const float4*> ( sc.tris );
    const float4* props = ( MODE == 1 && T ) ? T->l_props : reinterpret_cast<const float4*> ( sc.props );
    V3 ta, tb, tc; tri_vertices ( tris, ls.tri, ta, tb, tc );
    float4 p0 = props[4 * ls.tri + 0], p1 = props[4 * ls.tri + 1], p2 = props[4 * ls.tri + 2];
    // (the ray-sourced and lens units keep the plain root here: with the short one their LDS-resident Direct instances take 12 / 4 B more scratch than before,
    // profiles/short_sqrt/kernel_resources.md)
#if TERRA_RAY_SOURCE
    float s = sqrtf ( e1 );
#else
    float s = sqrt_exact ( e1 );
#endif
    float a = 1 - s, b = e2 * s, cw = 1 - a - b;
    ls.pos = ( ta * a + tb * b ) + tc * cw;
    V3 n = ( v3 ( p0.x, p0.y, p0.z ) * a + v3 ( p0.w, p1.x, p1.y ) * b ) + v3 ( p1.z, p1.w, p2.x ) * cw;
    ls.norm = normalize ( n );
    return ls;
}

// -----------------------------------------------------------------------------
// Environment importance sampling (extension, UNPINNED: nothing in the reference calls its TerraDistribution2D, src/Terra.c:812-846 -- the wiring is this
// repo's definition, restated by the oracle's environment_light_sample). One sample per shaded hit of Direct / Direct+MIS, after their own light samples: two draws of
// stream B pick a texel of the lat-long map through the table (e1: the row, e2: the column inside it; terra_distribution_2d_sample's arithmetic); the direction is the
// inverse of the lookup's mapping (src/Terra.c:468-477: theta = v terra_PI, phi = u 2 terra_PI - terra_PI); density over the sphere = texel probability x texels /
// (2 terra_PI^2 sin theta); the sample counts when the direction is in the upper hemisphere of the shading normal and its shadow ray leaves the scene; radiance = the
// chosen texel. Returns the term before the path throughput. Compiled into the KINDS & TERRA_KIND_SAMPLER kernels only.
// -----------------------------------------------------------------------------
TD bool env_sampling_active ( const DevScene& sc ) { return sc.env_nx != 0u; }
// with environment sampling in a light integrator the environment reaches a path through the samples taken at its hits: only the camera ray adds it on leaving the scene
template <int INTEGRATOR, int KINDS>
TD bool env_reaches_by_samples ( const DevScene& sc, uint32_t bounce ) {
    if constexpr ( ( KINDS & TERRA_KIND_SAMPLER ) != 0 && ( INTEGRATOR == 1 || INTEGRATOR == 2 ) ) return bounce != 0u && env_sampling_active ( sc );
    return false;
}
// environment MIS's lookup by direction: the texel environment_eval reads for `dir` (same mapping, same truncation; clamped into the table, which only a NaN
// direction can leave) and sin theta of `dir`
TD void environment_texel ( const DevScene& sc, V3 dir, uint32_t& col, uint32_t& row, float& st ) {
    const V3 d = normalize ( dir );
    const float theta = tdm_acosf ( d.y );
    const float phi = tdm_atan2f ( d.z, d.x ) + TERRA_PI_F;
    col = ( uint32_t ) ( ( phi / ( 2 * TERRA_PI_F ) ) * ( float ) sc.env_nx );
    row = ( uint32_t ) ( ( theta / TERRA_PI_F ) * ( float ) sc.env_ny );
    col = col < sc.env_nx - 1u ? col : sc.env_nx - 1u; row = row < sc.env_ny - 1u ? row : sc.env_ny - 1u;
    st = tdm_sinf ( theta );
}
// ... and the density over the sphere with which environment_light_sample produces a direction in that texel: the texel's probability in the table (bit-identical
// to the product of the two *pdf distribution_sample reports when it draws the texel) x texels / (2 terra_PI^2 sin theta), as environment_light_sample forms it;
// 0 where sin theta <= 0 or the texel cannot be drawn
TD float environment_texel_pdf ( const DevScene& sc, uint32_t col, uint32_t row, float st ) {
    const float prob = distribution_2d_prob ( sc.env_f, sc.env_row_f, sc.env_nx, sc.env_integral, row, col );
    if ( ! ( st > 0.f ) || ! ( prob > 0.f ) ) return 0.f;
    return prob * ( ( float ) sc.env_nx * ( float ) sc.env_ny ) / ( 2 * TERRA_PI_F * TERRA_PI_F * st );
}
TD float environment_pdf ( const DevScene& sc, V3 dir ) {
    uint32_t col, row; float st;
    environment_texel ( sc, dir, col, row, st );
    return environment_texel_pdf ( sc, col, row, st );
}
// lobes whose bsdf_eval is zero away from the direction their sampler chose (glass): the environment strategy adds nothing there, so under environment MIS the BSDF
// ray keeps its whole weight and the environment sample is left as it is
template <int KINDS>
TD bool bsdf_is_singular ( const Surface& sf ) { return ( KINDS & 8 ) && ( KINDS == 8 || sf.bsdf == kDevBsdfGlass ); }
// MIS: Direct + MIS in the environment-MIS variant (KINDS & TERRA_KIND_ENV_MIS) -- the term is weighted against the BSDF ray's density, p_e^2 / (p_e^2 + p_b^2), p_b read after the
// integrator's bsdf_sample (Phong's and glass's scratch slots hold that sample's choice). Same draws and the same shadow ray either way.
template <int COUNT, int MODE, int KINDS, bool MIS = false>
TD V3 environment_light_sample ( const Tracer& T, Surface& sf, V3 p, V3 wo, Pcg32& rb, Counters& c ) {
    const DevScene& sc = T.sc;
    const V3 zero = v3 ( 0, 0, 0 );
    const float e1 = randf ( rb, c, COUNT ), e2 = randf ( rb, c, COUNT );
    float p_row = 0.f, p_col = 0.f; uint32_t row = 0, col = 0;
    DevDistribution1D rows = { sc.env_row_f, sc.env_row_cdf, sc.env_ny, sc.env_integral, sc.env_monotone };
    const float sv = distribution_sample ( rows, e1, &p_row, &row );
    if ( sv == FLT_MAX ) return zero;
    DevDistribution1D cols = { sc.env_f + ( size_t ) sc.env_nx * row, sc.env_cdf + ( size_t ) sc.env_nx * row, sc.env_nx, sc.env_row_f[row], sc.env_monotone };
    const float su = distribution_sample ( cols, e2, &p_col, &col );
    if ( su == FLT_MAX ) return zero;
    const float theta = sv * TERRA_PI_F, phi = su * ( 2 * TERRA_PI_F ) - TERRA_PI_F;
    const float st = tdm_sinf ( theta ), ct = tdm_cosf ( theta ), sp = tdm_sinf ( phi ), cp = tdm_cosf ( phi );
    if ( ! ( st > 0.f ) ) return zero;
    const V3 wi = v3 ( st * cp, ct, st * sp );
    const float cosine = dot ( wi, sf.normal );
    if ( ! ( cosine > 0.f ) ) return zero;
    const float pdf = ( p_row * p_col ) * ( ( float ) sc.env_nx * ( float ) sc.env_ny ) / ( 2 * TERRA_PI_F * TERRA_PI_F * st );
    if ( ! ( pdf > 0.f ) ) return zero;
    Surface lsf;
    Ray r = surface_ray ( sf, p, wi );
    RaycastResult h = scene_raycast<COUNT, MODE, KINDS> ( T, r, lsf, c );
    if ( h.hit ) return zero;
    const V3 L = texture_read ( sc.textures[sc.env_tex], col, row );
    const V3 f = bsdf_eval<KINDS> ( sf, wi, wo );
    if constexpr ( MIS && ( KINDS & TERRA_KIND_ENV_MIS ) != 0 ) if ( !bsdf_is_singular<KINDS> ( sf ) ) {
        const float b = bsdf_pdf<KINDS> ( sf, wi, wo ), bpdf = b > 0.f ? b : 0.f;     // (Phong's lobe pdf is negative or NaN where the lobe is empty: density 0)
        const float r = bpdf / pdf, weight = 1.f / ( 1.f + r * r );                 // p_e^2 / (p_e^2 + p_b^2), defined when a density overflows
        return had ( L, f ) * ( cosine * weight / pdf );
    }
    return had ( L, f ) * ( cosine / pdf );
}

template <int COUNT, int MODE, int KINDS>
TD V3 integrate_direct ( const Tracer& T, Surface& sf, V3 p, V3 wo, V3 throughput, uint32_t bounce, Pcg32& rb, Counters& c ) {
    const DevScene& sc = T.sc;
    V3 Lo = v3 ( 0, 0, 0 );
    if ( bounce == 0 && dot ( wo, sf.normal ) > 0 ) Lo = Lo + sf.emissive;
    LightSample ls = draw_light_sample<COUNT, MODE> ( sc, rb, c, &T );
    V3 p_to_light = ls.pos - p;
    V3 wi = normalize ( p_to_light );
    Surface lsf;
    Ray r = surface_ray ( sf, p, wi );
    RaycastResult h = scene_raycast<COUNT, MODE, KINDS> ( T, r, lsf, c );
    if ( h.hit && h.object == ls.light_object && h.tri_in_object == ls.tri_in_object ) {
        float cosv = dot ( neg ( wi ), ls.norm );
        if ( cosv > 0 ) {
            V3 f = bsdf_eval<KINDS> ( sf, wi, wo );
            float pdf = dot ( p_to_light, p_to_light ) / fabsf ( cosv * T.l_area[h.tri] );
            V3 Ld = had ( lsf.emissive, f );
            Ld = Ld * ( dot ( wi, sf.normal ) / ( pdf * ls.pick_pdf ) );
            Lo = Lo + Ld;
        }
    }
    if constexpr ( ( KINDS & TERRA_KIND_SAMPLER ) != 0 ) { if ( env_sampling_active ( sc ) ) Lo = Lo + environment_light_sample<COUNT, MODE, KINDS> ( T, sf, p, wo, rb, c ); }
    return had ( Lo, throughput );
}

// integrate_direct split at its shadow ray, for the decoupled loop (render_kernels.hip): everything that does not depend
// on the shadow ray's outcome is done up front -- same operations in the same order -- and both possible return values
// are kept: `hid` (light sample not visible) and `vis` (visible). Valid for scenes without textured attributes, where the
// emissive the shadow ray's surface_init would read is the light material's constant.
struct DirectPending { V3 vis, hid; uint32_t expected; };
// MODE: where the light's triangle, the materials and the areas are read from (1: the block's LDS copies, through T.l_*)
template <int COUNT, int KINDS, int MODE = 0>
TD DirectPending direct_prepare ( const Tracer& T, Surface& sf, V3 p, V3 wo, V3 throughput, uint32_t bounce, Pcg32& rb, Counters& c, Ray& shadow_ray ) {
    const DevScene& sc = T.sc;
    V3 Lo = v3 ( 0, 0, 0 );
    if ( bounce == 0 && dot ( wo, sf.normal ) > 0 ) Lo = Lo + sf.emissive;
    LightSample ls = draw_light_sample<COUNT, MODE> ( sc, rb, c, &T );
    V3 p_to_light = ls.pos - p;
    V3 wi = normalize ( p_to_light );
    shadow_ray = surface_ray ( sf, p, wi );
    DirectPending d;
    d.hid = had ( Lo, throughput ); d.vis = d.hid; d.expected = ls.tri;
    float cosv = dot ( neg ( wi ), ls.norm );
    if ( cosv > 0 ) {
        V3 f = bsdf_eval<KINDS> ( sf, wi, wo );
        float pdf = dot ( p_to_light, p_to_light ) / fabsf ( cosv * T.l_area[ls.tri] );
        V3 Ld = had ( v3p ( T.l_mats[ls.light_object].emissive ), f );
        Ld = Ld * ( dot ( wi, sf.normal ) / ( pdf * ls.pick_pdf ) );
        d.vis = had ( Lo + Ld, throughput );
    }
    return d;
}

// integrate_mis (DEBUG_WEIGHTS = false) split at its two rays, for the decoupled loop. mis_prepare does everything that
// precedes the light-sample shadow ray (job A) and prepares both of its outcomes as the integrator's running sum
// (a_hid: emissive term only; a_vis: + the light-sample term); it also evaluates what the BSDF-sample ray (job B) will
// need from the shaded surface. mis_finish_b applies job B's hit to the running sum exactly as integrate_mis does.
// Job A's visible term uses the light material's constant emissive: valid for scenes without textured attributes.
struct MisPending { V3 a_vis, a_hid; uint32_t expected; V3 f2; float bpdf2, cos2; V3 p; uint32_t light_object; V3 t_before; };
template <int COUNT, int KINDS, int MODE = 0>
TD MisPending mis_prepare ( const Tracer& T, Surface& sf, V3 p, V3 wo, V3 throughput, uint32_t bounce, Pcg32& rb, Counters& c, Ray& ray_a, V3& dir_b ) {
    const DevScene& sc = T.sc;
    V3 Lo = v3 ( 0, 0, 0 );
    if ( bounce == 0 && dot ( wo, sf.normal ) > 0 ) Lo = Lo + sf.emissive;
    const float e1 = randf ( rb, c, COUNT ); const uint32_t k2 = randf_bits ( rb, c, COUNT ); const float e2 = trng_b_from_bits ( k2 ), e3 = randf ( rb, c, COUNT );
    V3 bsdf_dir = bsdf_sample<KINDS> ( sf, e1, e2, e3, wo, azimuth_fetch_index ( azimuth_table<MODE> ( sc ), k2 ) );
    LightSample ls = draw_light_sample<COUNT, MODE> ( sc, rb, c, &T );
    MisPending m;
    m.a_hid = Lo; m.a_vis = Lo; m.expected = ls.tri; m.p = p; m.light_object = ls.light_object; m.t_before = throughput;
    {
        V3 p_to_light = ls.pos - p;
        V3 wi = normalize ( p_to_light );
        ray_a = surface_ray ( sf, p, wi );
        float cosv = dot ( ls.norm, neg ( wi ) );
        if ( cosv > 0 ) {
            float bpdf = bsdf_pdf<KINDS> ( sf, wi, wo );
            float lpdf = dot ( p_to_light, p_to_light ) / fabsf ( cosv * T.l_area[ls.tri] );
            float weight = ( lpdf * lpdf ) / ( lpdf * lpdf + bpdf * bpdf );
            if ( lpdf != 0 ) {
                V3 f = bsdf_eval<KINDS> ( sf, wi, wo );
                V3 L = had ( v3p ( T.l_mats[ls.light_object].emissive ), f );
                L = L * ( dot ( wi, sf.normal ) * weight / ( lpdf * ls.pick_pdf ) );
                m.a_vis = Lo + L;
            }
        }
    }
    dir_b = bsdf_dir;
    m.f2 = bsdf_eval<KINDS> ( sf, bsdf_dir, wo );
    m.bpdf2 = bsdf_pdf<KINDS> ( sf, bsdf_dir, wo );
    m.cos2 = dot ( bsdf_dir, sf.normal );
    return m;
}
// job B came back with closest hit (tri, point, shaded surface lsf of the hit): returns the integrator's value
template <int MODE>
TD V3 mis_finish_b ( const Tracer& T, const MisPending& m, V3 Lo, bool hit, uint32_t hit_object, uint32_t hit_tri, V3 hit_point, const Surface& lsf, V3 wi ) {
    if ( hit && hit_object == m.light_object ) {
        float NoW = dot ( lsf.normal, neg ( wi ) );
        if ( NoW > 0 ) {
            V3 dl = m.p - hit_point;
            float dist = dot ( dl, dl );
            const float4* tris = MODE == 1 ? reinterpret_cast<const float4*> ( T.l_tris ) : reinterpret_cast<const float4*> ( T.sc.tris );      // (hit_tri: index in the soup)
            V3 ta, tb, tc; tri_vertices ( tris, hit_tri, ta, tb, tc );
            float area = triangle_area ( ta, tb, tc );
            float lpdf = dist / ( NoW * area );
            float weight = ( m.bpdf2 * m.bpdf2 ) / ( lpdf * lpdf + m.bpdf2 * m.bpdf2 );
            if ( m.bpdf2 != 0 ) {
                V3 L = had ( lsf.emissive, m.f2 );
                L = L * ( m.cos2 * weight / m.bpdf2 );
                Lo = Lo + L;
            }
        }
    }
    return had ( Lo, m.t_before );
}

template <int COUNT, int MODE, int KINDS, bool DEBUG_WEIGHTS>
TD V3 integrate_mis ( const Tracer& T, Surface& sf, V3 p, V3 wo, V3 throughput, uint32_t bounce, Pcg32& rb, Counters& c ) {
    const DevScene& sc = T.sc;
    V3 Lo = v3 ( 0, 0, 0 );
    if ( DEBUG_WEIGHTS ) { if ( bounce != 0 ) return Lo; }
    else if ( bounce == 0 && dot ( wo, sf.normal ) > 0 ) Lo = Lo + sf.emissive;
    const float e1 = randf ( rb, c, COUNT ); const uint32_t k2 = randf_bits ( rb, c, COUNT ); const float e2 = trng_b_from_bits ( k2 ), e3 = randf ( rb, c, COUNT );
    V3 bsdf_dir = bsdf_sample<KINDS> ( sf, e1, e2, e3, wo, azimuth_fetch_index ( azimuth_table<MODE> ( sc ), k2 ) );
    LightSample ls = draw_light_sample<COUNT, MODE> ( sc, rb, c, &T );
    {
        V3 p_to_light = ls.pos - p;
        V3 wi = normalize ( p_to_light );
        Surface lsf;
        Ray r = surface_ray ( sf, p, wi );
        RaycastResult h = scene_raycast<COUNT, MODE, KINDS> ( T, r, lsf, c );
        if ( h.hit && h.object == ls.light_object && h.tri_in_object == ls.tri_in_object ) {
            float cosv = dot ( ls.norm, neg ( wi ) );
            if ( cosv > 0 ) {
                float bpdf = bsdf_pdf<KINDS> ( sf, wi, wo );
                float lpdf = dot ( p_to_light, p_to_light ) / fabsf ( cosv * T.l_area[h.tri] );
                if ( DEBUG_WEIGHTS ) {
                    float weight = ( bpdf * bpdf ) / ( lpdf * lpdf + bpdf * bpdf );
                    Lo = Lo + v3 ( 0, 0, weight );
                } else {
                    float weight = ( lpdf * lpdf ) / ( lpdf * lpdf + bpdf * bpdf );
                    if ( lpdf != 0 ) {
                        V3 f = bsdf_eval<KINDS> ( sf, wi, wo );
                        V3 L = had ( lsf.emissive, f );
                        L = L * ( dot ( wi, sf.normal ) * weight / ( lpdf * ls.pick_pdf ) );
                        Lo = Lo + L;
                    }
                }
            }
        }
    }
    {
        V3 wi = bsdf_dir;
        V3 f = bsdf_eval<KINDS> ( sf, wi, wo );
        float bpdf = bsdf_pdf<KINDS> ( sf, wi, wo );
        V3 light_wo = neg ( wi );
        Surface lsf;
        Ray r = surface_ray ( sf, p, wi );
        RaycastResult h = scene_raycast<COUNT, MODE, KINDS> ( T, r, lsf, c );
        if ( h.hit && h.object == ls.light_object ) {
            float NoW = dot ( lsf.normal, light_wo );
            if ( NoW > 0 ) {
                V3 dl = p - h.point;
                float dist = dot ( dl, dl );
                const float4* tris = reinterpret_cast<const float4*> ( sc.tris );
                V3 ta, tb, tc; tri_vertices ( tris, h.tri, ta, tb, tc );
                float area = triangle_area ( ta, tb, tc );
                float lpdf = dist / ( NoW * area );
                float weight = ( bpdf * bpdf ) / ( lpdf * lpdf + bpdf * bpdf );
                if ( DEBUG_WEIGHTS ) {
                    Lo = Lo + v3 ( weight, 0, 0 );
                } else if ( bpdf != 0 ) {
                    V3 L = had ( lsf.emissive, f );
                    L = L * ( dot ( wi, sf.normal ) * weight / bpdf );
                    Lo = Lo + L;
                }
            }
        }
        if constexpr ( ( KINDS & TERRA_KIND_ENV_MIS ) != 0 && !DEBUG_WEIGHTS ) {
            // environment MIS: the BSDF ray that leaves the scene sees the environment, weighted against the density with which the environment sample could
            // have produced its direction (0 below the shading normal's horizon and for singular lobes: weight 1)
            if ( !h.hit && bpdf > 0.f ) {         // (skips p_b = 0 like the area-light branch, and a negative or NaN lobe pdf)
                uint32_t col, row; float st;
                environment_texel ( sc, wi, col, row, st );          // (environment_eval's texel: one lookup serves the radiance and the density)
                const float epdf = ( !bsdf_is_singular<KINDS> ( sf ) && dot ( wi, sf.normal ) > 0 ) ? environment_texel_pdf ( sc, col, row, st ) : 0.f;
                const float r = epdf / bpdf, weight = 1.f / ( 1.f + r * r );        // p_b^2 / (p_b^2 + p_e^2), defined when a density overflows
                V3 L = had ( texture_read ( sc.textures[sc.env_tex], col, row ), f );
                L = L * ( dot ( wi, sf.normal ) * weight / bpdf );
                Lo = Lo + L;
            }
        }
    }
    if constexpr ( ( KINDS & TERRA_KIND_SAMPLER ) != 0 && !DEBUG_WEIGHTS ) { if ( env_sampling_active ( sc ) ) Lo = Lo + environment_light_sample<COUNT, MODE, KINDS, true> ( T, sf, p, wo, rb, c ); }
    return had ( Lo, throughput );
}

TD V3 integrate_debug_normals ( const Surface& sf, uint32_t bounce ) {
    if ( bounce != 0 ) return v3 ( 0, 0, 0 );
    V3 n = sf.normal;
    V3 pp = v3 ( sel_min ( n.x > 0 ? n.x : 0.f, 1.f ), sel_min ( n.y > 0 ? n.y : 0.f, 1.f ), sel_min ( n.z > 0 ? n.z : 0.f, 1.f ) );
    V3 nn = v3 ( sel_min ( n.x > -1 ? n.x : -1.f, 0.f ), sel_min ( n.y > -1 ? n.y : -1.f, 0.f ), sel_min ( n.z > -1 ? n.z : -1.f, 0.f ) );
    nn = nn * -1.f;
    V3 col = v3 ( 0, 0, 0 );
    col = col + v3 ( 1, 0, 0 ) * pp.x;
    col = col + v3 ( 0, 1, 0 ) * pp.y;
    col = col + v3 ( 0, 0, 1 ) * pp.z;
    col = col + v3 ( 0, 1, 1 ) * nn.x;
    col = col + v3 ( 1, 0, 1 ) * nn.y;
    col = col + v3 ( 1, 1, 0 ) * nn.z;
    return col;
}

// integrator ids = TerraIntegrator (reference include/Terra.h:149-157)
template <int INTEGRATOR, int COUNT, int MODE, int KINDS>
TD V3 integrate ( const Tracer& T, const Ray& ray, Surface& sf, V3 p, V3 wo, V3 throughput, uint32_t bounce, Pcg32& rb, Counters& c ) {
    if ( INTEGRATOR == 0 ) {
        if ( dot ( wo, sf.normal ) > 0 ) return had ( sf.emissive, throughput );
        return v3 ( 0, 0, 0 );
    } else if ( INTEGRATOR == 1 ) {
        return integrate_direct<COUNT, MODE, KINDS> ( T, sf, p, wo, throughput, bounce, rb, c );
    } else if ( INTEGRATOR == 2 ) {
        return integrate_mis<COUNT, MODE, KINDS, false> ( T, sf, p, wo, throughput, bounce, rb, c );
    } else if ( INTEGRATOR == 3 ) {
        return bounce != 0 ? v3 ( 0, 0, 0 ) : v3 ( 1, 1, 1 );
    } else if ( INTEGRATOR == 4 ) {
        if ( bounce != 0 ) return v3 ( 0, 0, 0 );
        float d = length ( ray.o - p ) / 500.f;
        return v3 ( d, d, d );
    } else if ( INTEGRATOR == 5 ) {
        return integrate_debug_normals ( sf, bounce );
    } else {
        return integrate_mis<COUNT, MODE, KINDS, true> ( T, sf, p, wo, throughput, bounce, rb, c );
    }
}

// The tail of one terra_trace iteration after the integrator's term (reference src/Terra.c:1066-1094): sample the BSDF, weight the
// throughput, play Russian roulette. Returns true when the path goes on (then `bounce` was advanced and wi is the next direction; the
// caller forms the next ray from the hit point). Same operations, draws and order in all four loops of the kernel.
// The four variates are consecutive draws of stream B whatever the surface is, so they can be drawn -- and the azimuth table entry requested -- BEFORE the
// surface is set up (path_draw), which hides the load behind terra_surface_init's work; integrators that draw from the stream themselves (Direct, MIS) call
// path_draw after their own draws, as the reference's order demands.
// The azimuth is the second variate's: e1 = k * 2^-24 exactly (k < 2^24 is a float, and so is the product), and the integer is still here, so the azimuth takes it
template <int COUNT>
TD PathDraws path_draw ( const float2* sincos24, Pcg32& rb, Counters& c ) {
    PathDraws d;
    d.e0 = randf ( rb, c, COUNT );
    const uint32_t k1 = randf_bits ( rb, c, COUNT );
    d.e1 = trng_b_from_bits ( k1 );
    d.e2 = randf ( rb, c, COUNT );
    d.az = azimuth_fetch_index ( sincos24, k1 );
    d.e3 = randf ( rb, c, COUNT );
    return d;
}
// (restated for a diffuse surface in continue_stage below: a change here goes into both)
template <int KINDS>
TD bool path_continue ( Surface& sf, V3 wo, V3& throughput, uint32_t& bounce, uint32_t max_bounces, const PathDraws& d, V3& wi ) {
    wi = bsdf_sample<KINDS> ( sf, d.e0, d.e1, d.e2, wo, d.az );
    float pdf = sel_max ( bsdf_pdf<KINDS> ( sf, wi, wo ), ( float ) 1e-4 );
    V3 f = bsdf_eval<KINDS> ( sf, wi, wo ) * rcp_exact ( pdf );
    throughput = had ( throughput, f );
    throughput = throughput * dot ( sf.normal, wi );
    float pr = sel_max ( throughput.x, sel_max ( throughput.y, throughput.z ) );
    if ( d.e3 > pr ) return false;
        throughput = throughput * roulette_scale ( pr );          // ( float ) ( 1.0 / ( ( double ) pr + 1e-4 ) ), bit for bit (exact_div.h)
    ++bounce;
    return bounce <= max_bounces;
}
// Stage S3 of the shading stages (exact_div.h "Shading stages"): path_continue<1> of a diffuse surface from the BSDF sample to the roulette's rescale, nine sites --
// diffuse_sample's two roots, make_basis's root, the normalisation of wi (a root and the quotients), diffuse_pdf's quotient, rcp_exact ( pdf ), roulette_scale.
// Same operations in the same order as path_continue<1>; the draws were made before (path_draw), so no stream moves when the stage runs twice. Nothing is committed
// here: the outputs are wi, the new throughput t and go = "the roulette let the path live"; the caller writes them after its vote. Returns the lane's mask.
// SHORT = false, DROPS = false: path_continue<1>'s own helpers, guard for guard. DROPS: d.e0 is a stream-B variate (exact_sqrt.h xs_variate_ok) and the
// density is clamped (exact_div.h xd_rcp_clamped_ok); the direction wi keeps every test when it becomes the next ray (trace_math.h ray_stage). Kept: the tests of the tangent frame's and wi's roots and components, of diffuse_pdf's numerator
// (a grazing wi makes it 0) and roulette_scale's bounds.
template <bool SHORT, bool DROPS>
TD int continue_stage ( V3 n, V3 albedo, V3 throughput, const PathDraws& d, V3& wi, V3& t, bool& go ) {
    int ok = 1;
    const float r = xs_site_sqrt<SHORT> ( d.e0, DROPS ? xs_variate_ok ( d.e0 ) : xs_in_range ( d.e0 ), ok );
    float sn, cs;
    azimuth_sincos ( d.az, d.e1, sn, cs );
    const float x = r * cs, z = r * sn;
    const float om = sel_max ( 0.f, 1 - d.e0 );
    const float y = xs_site_sqrt<SHORT> ( om, DROPS ? 1 : xs_in_range ( om ), ok );
    wi = normalize_site<SHORT> ( basis_apply ( make_basis_site<SHORT> ( n, ok ), v3 ( x, y, z ) ), ok );
    const float pdf = sel_max ( xd_site_div_rk<SHORT> ( sel_max ( 0.f, dot ( n, wi ) ), TERRA_PI_F, TERRA_INV_PI_F, ok ), ( float ) 1e-4 );
    const V3 f = ( albedo * ( float ) ( 1. / ( double ) TERRA_PI_F ) ) * xd_site_rcp<SHORT> ( pdf, DROPS ? xd_rcp_clamped_ok ( pdf ) : xd_rcp_ok ( pdf ), ok );
    t = had ( throughput, f );
    t = t * dot ( n, wi );
    const float pr = sel_max ( t.x, sel_max ( t.y, t.z ) );
    go = ! ( d.e3 > pr );
    if constexpr ( SHORT ) {          // (a path the roulette ends keeps its throughput unscaled, as path_continue leaves it: t * 1.f is t)
        ok &= roulette_scale_ok ( pr ) | ( int ) !go;
        t = t * ( go ? roulette_scale_short ( pr ) : 1.f );
    } else if ( go ) t = t * roulette_scale ( pr );
    return ok;
}
// path_continue<1> for the kernels of ray_start_masks_for: the stage, one vote, the guarded helpers for a wave that holds a lane some guard turned away; then the commit
TD bool path_continue_staged ( const Surface& sf, V3& throughput, uint32_t& bounce, uint32_t max_bounces, const PathDraws& d, V3& wi ) {
    V3 t; bool go;
    if constexpr ( TERRA_SHADE_STAGES != 0 ) {
        if ( __any ( !continue_stage<true, TERRA_SHADE_DROPS != 0> ( sf.normal, sf.attr[0], throughput, d, wi, t, go ) ) )
            continue_stage<false, false> ( sf.normal, sf.attr[0], throughput, d, wi, t, go );
    } else continue_stage<false, TERRA_SHADE_DROPS != 0> ( sf.normal, sf.attr[0], throughput, d, wi, t, go );
    throughput = t;
    if ( !go ) return false;
    ++bounce;
    return bounce <= max_bounces;
}
// Sampler integration (terra_amd_set_sampler_integration, UNPINNED extension): at bounce 0 the pixel sampler's pair replaces the first two variates handed to
// the BSDF's sampler; stream B has been consumed as always
struct SamplerPair { float u0, u1; bool on; };
TD SamplerPair sampler_pair_none() { SamplerPair s; s.u0 = s.u1 = 0.f; s.on = false; return s; }
TD void path_apply_sampler ( PathDraws& d, const SamplerPair& sp, uint32_t bounce ) {
    if ( sp.on && bounce == 0 ) { d.e0 = sp.u0; d.e1 = sp.u1; d.az = azimuth_none(); }
}
// element n of the pixel's sampler (n = camera samples the pixel has received before this one), as the oracle's orc_render_pixels takes it: Halton = the
// radical-inverse pair of n (src/Terra.c:734-755); stratified = the sampler of src/Terra.c:542 at element n mod (strata^2 * 16), its two offsets the next draws of
// the pixel's camera stream (src/Terra.c:714-723)
TD SamplerPair sampler_pair_draw ( uint32_t mode, uint32_t strata, uint64_t n, Pcg32& stream_a ) {
    SamplerPair s = sampler_pair_none();
    if ( mode == 1 ) { s.u0 = radical_inverse ( 3, n ); s.u1 = radical_inverse ( 2, n ); s.on = true; }
    else if ( mode == 2 && strata > 0 ) {
        const uint64_t cap = ( uint64_t ) strata * strata * 16ull, m = n % cap, stratum = m / 16ull;
        const float stratum_size = 1.f / ( float ) strata;
        s.u0 = sd_below_one ( ( ( float ) ( uint32_t ) ( stratum % strata ) + trng_a_float ( stream_a ) ) * stratum_size );
        s.u1 = sd_below_one ( ( ( float ) ( uint32_t ) ( stratum / strata ) + trng_a_float ( stream_a ) ) * stratum_size );
        s.on = true;
    }
    return s;
}
template <int COUNT, int KINDS>
TD bool path_continue ( const DevScene& sc, Surface& sf, V3 wo, V3& throughput, uint32_t& bounce, uint32_t max_bounces, Pcg32& rb, Counters& c, V3& wi, const SamplerPair& sp = sampler_pair_none() ) {
    PathDraws d = path_draw<COUNT> ( sc.sincos24, rb, c );
    if ( KINDS & TERRA_KIND_SAMPLER ) path_apply_sampler ( d, sp, bounce );
    return path_continue<KINDS> ( sf, wo, throughput, bounce, max_bounces, d, wi );
}

// -----------------------------------------------------------------------------
// one full path (the reference's terra_trace), used by the unit entry point and,
// restructured with path regeneration, by the render kernel
// -----------------------------------------------------------------------------
template <int INTEGRATOR, int COUNT, int MODE, int KINDS>
TD V3 trace_path ( const Tracer& T, Ray ray, uint32_t bounces, Pcg32& rb, Counters& c ) {
    V3 Lo = v3 ( 0, 0, 0 ), throughput = v3 ( 1, 1, 1 );
    for ( uint32_t bounce = 0; bounce <= bounces; ++bounce ) {
        Surface sf;
        RaycastResult h = scene_raycast<COUNT, MODE, KINDS> ( T, ray, sf, c );
        if ( !h.hit ) {
            if ( ( KINDS & TERRA_KIND_ENV ) && T.sc.env_mode && !env_reaches_by_samples<INTEGRATOR, KINDS> ( T.sc, bounce ) ) { throughput = had ( throughput, environment_eval ( T.sc, ray.d ) ); Lo = Lo + throughput; }
            break;
        }
        V3 wo = neg ( ray.d );
        Lo = Lo + integrate<INTEGRATOR, COUNT, MODE, KINDS> ( T, ray, sf, h.point, wo, throughput, bounce, rb, c );
        V3 wi;
        uint32_t next_bounce = bounce;
        if ( !path_continue<COUNT, KINDS> ( T.sc, sf, wo, throughput, next_bounce, bounces, rb, c, wi ) ) break;
        ray = surface_ray ( sf, h.point, wi );
    }
    return Lo;
}

// -----------------------------------------------------------------------------
// tonemap
// -----------------------------------------------------------------------------
TD V3 uncharted2 ( V3 x ) {
    const float A = 0.15f, B = 0.5f, C = 0.1f, D = 0.2f, E = 0.02f, F = 0.3f;
    V3 r;
    r.x = ( ( x.x * ( A * x.x + C * B ) + D * E ) / ( x.x * ( A * x.x + B ) + D * F ) ) - E / F;
    r.y = ( ( x.y * ( A * x.y + C * B ) + D * E ) / ( x.y * ( A * x.y + B ) + D * F ) ) - E / F;
    r.z = ( ( x.z * ( A * x.z + C * B ) + D * E ) / ( x.z * ( A * x.z + B ) + D * F ) ) - E / F;
    return r;
}
TD V3 powv ( V3 c, float e ) { return v3 ( tdm_powf ( c.x, e ), tdm_powf ( c.y, e ), tdm_powf ( c.z, e ) ); }
TD V3 tonemap ( V3 c, int op, float gamma ) {
    switch ( op ) {
        case 1: c = powv ( c, 1.f / gamma ); break;
        case 2:
            c.x = c.x / ( 1.f + c.x ); c.y = c.y / ( 1.f + c.y ); c.z = c.z / ( 1.f + c.z );
            c = powv ( c, 1.f / gamma ); break;
        case 3: {
            V3 x = v3 ( sel_max ( 0.f, c.x - 0.004f ), sel_max ( 0.f, c.y - 0.004f ), sel_max ( 0.f, c.z - 0.004f ) );
            c.x = ( x.x * ( 6.2f * x.x + 0.5f ) ) / ( x.x * ( 6.2f * x.x + 1.7f ) + 0.06f );
            c.y = ( x.y * ( 6.2f * x.y + 0.5f ) ) / ( x.y * ( 6.2f * x.y + 1.7f ) + 0.06f );
            c.x = ( x.z * ( 6.2f * x.z + 0.5f ) ) / ( x.z * ( 6.2f * x.z + 1.7f ) + 0.06f );   // the reference stores the .z curve in .x
            break;
        }
        case 4: {
            V3 ws = uncharted2 ( v3 ( 11.2f, 11.2f, 11.2f ) );
            ws = v3 ( 1.f / ws.x, 1.f / ws.y, 1.f / ws.z );
            V3 t = uncharted2 ( c * 2.f );
            c = powv ( had ( t, ws ), 1.f / gamma );
            break;
        }
        default: break;
    }
    return c;
}
