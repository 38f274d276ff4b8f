/*
 * terra_headless -- OBJ/MTL in, PNG/PPM/PFM/HDR out, through the Terra.h API only.
 *
 * the headless counterpart of the reference's GUI client for this
 * path -- mesh -> TerraObject fill and material mapping (satellite/src/Scene.cpp:133-245:
 * one object per mesh/material, specular materials -> Phong preset, everything else ->
 * diffuse; right-handed OBJ -> left-handed Terra by flipping z and the winding,
 * Scene.cpp:90-93) and image export (satellite/src/Visualization.cpp:286-357: clamp x 255
 * for PNG, raw floats for HDR). It links against libterra_amd.so or, unchanged, against the
 * reference's objects (only Terra.h / TerraPresets.h symbols are used; terra_amd_* are weak).
 *
 * Import policy (--normals apollo, the default): the reference's client imports OBJ with its Apollo importer
 * (satellite/include/Apollo.h:964-1700) under the options of satellite/src/Scene.cpp:83-93 -- recompute_vertex_normals,
 * remove_vertex_duplicates, flip_z, flip_faces_winding_order. Apollo.h does not compile with this image's toolchains, so its
 * policy is RESTATED here and pinned by hand-derived fixtures (tests/test_headless_tool.py), not by running it:
 *   - one object per `g` / `o` group (a group is opened implicitly by the first `usemtl`, `s` or `f`); the group's material is
 *     the LAST `usemtl` inside it; the material's class is the word of Apollo's own `illum <word>` dialect (Apollo.h:877-897) and only
 *     `illum specular` selects Phong: diffuse, mirror, pbr, disney and materials without such a word (every standard MTL file, whose
 *     `illum 2` Apollo rejects) become diffuse, the last four with a warning, as satellite/src/Scene.cpp:193-230 does; Ke is the emissive;
 *   - z is negated at parse time and every triangle (a, b, c) becomes (c, b, a);
 *   - the file's `vn` are ignored. Face normal = normalize(cross(v1 - v0, v2 - v0)) of the flipped triangle. A group is smooth
 *     iff its last `s` token starts with '1'; in smooth groups corners with bit-equal positions share one vertex (the first one
 *     created anywhere in the file) and its first texcoord. A vertex normal is the normalised, unweighted sum of the face
 *     normals of the triangles the vertex was PARSED for: corners 0-2 of a polygon count for its first triangle only, corner
 *     j >= 3 for triangle j - 2 (Apollo records adjacency per parsed corner, Apollo.h:1373-1381); `s off` / `s 0` groups get
 *     the face normal per triangle; groups without any `s` take the smooth path without sharing, i.e. face normals again.
 * --normals file keeps the file's `vn` (area-weighted smooth normals per position where absent), one object per material, and reads
 * standard MTL files the usual way (Ks > 0 -> Phong when there is no Apollo `illum` word): this repo's own policy, not the reference's.
 *
 *   terra_headless scene.obj out.png [--width W] [--height H] [--spp N] [--bounces N]
 *       [--integrator simple|direct|mis|normals|depth] [--tonemap none|linear|reinhard|filmic|uncharted2]
 *       [--camera px py pz dx dy dz] [--fov deg] [--exposure e] [--gamma g] [--jitter j]
 *       [--no-flip-z] [--normals apollo|file] [--dump-scene file] [--no-render] [--fast-tree | --replica-tree] [--sample-split n] [--seed n] [--tile n] [--gpus n]
 *       [--environment map.hdr|map.pfm] [--environment-color r g b] [--env-light] [--env-sampling off|table|mis] [--aov PREFIX] [--denoise K]
 *       [--passes N] [--denoise-variance K] [--adaptive TARGET [--min-passes A] [--max-passes B] [--adaptive-masked]] [--variance out.pfm]
 *       [--frames N] [--camera-to px py pz dx dy dz] [--temporal ALPHA]
 *       [--camera-model pinhole|thinlens|ortho|equirect|fisheye] [--aperture R] [--focus D] [--ortho-height H] [--fisheye-fov DEG]
 *       [--bake-lightmap [--atlas WxH] [--bake-margin M] [--bake-dilate N]]
 *       [--bake-probes NXxNYxNZ [--probe-cells N] [--probe-visibility maps.pfm [--probe-texels M]]]
 *       [--distance-field NXxNYxNZ field.pfm [--signed]]
 *
 * Environment: the scene's environment attribute is a constant (--environment-color, default 0.4 0.52 1) or a lat-long map (--environment: Radiance .hdr with flat
 * or new-style run-length-encoded scanlines, orientation -Y H +X W, texel = m 2^(e - 136); or .pfm, either byte order, bottom row first), bound as a 3-component
 * float texture with terra_attribute_init_cubemap. The reference drops the environment term; libterra_amd.so adds it with --env-light, samples the map with
 * --env-sampling table (a TerraDistribution2D over the map) and weights that sample against Direct + MIS's BSDF ray with --env-sampling mis.
 */
#include <ctype.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "Terra.h"
#include "TerraPresets.h"

const char* terra_amd_last_error ( void ) __attribute__ ( ( weak ) );
int         terra_amd_set_tree_mode ( HTerraScene, int ) __attribute__ ( ( weak ) );
int         terra_amd_set_sample_split ( HTerraScene, int ) __attribute__ ( ( weak ) );
void        terra_amd_set_frame_seed ( HTerraScene, uint64_t ) __attribute__ ( ( weak ) );
uint64_t    terra_amd_get_frame_seed ( HTerraScene ) __attribute__ ( ( weak ) );
int         terra_amd_init ( void ) __attribute__ ( ( weak ) );
int         terra_amd_set_devices ( const int*, int ) __attribute__ ( ( weak ) );
int         terra_amd_device_count ( void ) __attribute__ ( ( weak ) );
int         terra_amd_render_multi ( const TerraCamera*, HTerraScene, const TerraFramebuffer*, size_t, size_t, size_t, size_t, size_t ) __attribute__ ( ( weak ) );
int         terra_amd_set_environment_lighting ( HTerraScene, int ) __attribute__ ( ( weak ) );
int         terra_amd_set_environment_sampling ( HTerraScene, int ) __attribute__ ( ( weak ) );
int         terra_amd_set_environment_mis ( HTerraScene, int ) __attribute__ ( ( weak ) );
/* first-hit AOV sums (TerraAmdAovResult of terra_amd.h, restated: this file also builds against the reference's headers) and the denoiser */
typedef struct { float albedo[3]; float coverage; float normal[3]; float depth; int samples; int reserved[3]; } AovSum;
int         terra_amd_render_aov ( const TerraCamera*, HTerraScene, void*, size_t, size_t, size_t, size_t, size_t, size_t ) __attribute__ ( ( weak ) );
int         terra_amd_denoise ( HTerraScene, const TerraFramebuffer*, const void*, size_t, size_t, size_t, size_t, int, TerraFloat3*, TerraFloat3* ) __attribute__ ( ( weak ) );
/* per-pixel second moments (TerraAmdMoments, TerraAmdAdaptiveOptions / Report of terra_amd.h, restated for the same reason), their denoiser and the adaptive driver */
typedef struct { float seen_acc[3]; int seen_samples; float mean; float m2; int batches; int weight; } MomentSum;
typedef struct { size_t tile_size; int min_batches; int max_batches; float target_error; int reserved; } AdaptiveOptions;
typedef struct { int rounds; int hit_max_batches; int tiles; int tiles_converged; uint64_t tile_calls; uint64_t samples; float max_error; int reserved; } AdaptiveReport;
int         terra_amd_accumulate_moments ( HTerraScene, const TerraFramebuffer*, void*, size_t, size_t, size_t, size_t ) __attribute__ ( ( weak ) );
int         terra_amd_denoise_variance ( HTerraScene, const TerraFramebuffer*, const void*, const void*, size_t, size_t, size_t, size_t, int, TerraFloat3*, TerraFloat3* ) __attribute__ ( ( weak ) );
int         terra_amd_render_adaptive ( const TerraCamera*, HTerraScene, TerraFramebuffer*, void*, void*, size_t, size_t, size_t, size_t, const void*, void* ) __attribute__ ( ( weak ) );
int         terra_amd_render_adaptive_masked ( const TerraCamera*, HTerraScene, TerraFramebuffer*, void*, void*, size_t, size_t, size_t, size_t, const void*, void* ) __attribute__ ( ( weak ) );

/* the per-pixel history of the temporal reprojection (TerraAmdHistory, TerraAmdTemporalOptions of terra_amd.h, restated for the same reason) */
typedef struct { float radiance[3]; float length; float normal[3]; float depth; float mu1, mu2; float reserved[2]; } HistoryEntry;
typedef struct { float alpha; float depth_tolerance; float normal_cos; int reserved; } TemporalOptions;
int         terra_amd_reproject ( HTerraScene, const TerraCamera*, const TerraCamera*, const TerraFramebuffer*, const void*, const void*, void*, void*, void*,
                                  size_t, size_t, size_t, size_t, const void* ) __attribute__ ( ( weak ) );

/* camera models (TerraAmdLens and the lens calls of terra_amd.h "Lens rendering", restated for the same reason) */
typedef struct { int model; float lens_radius, focus_distance, ortho_height, fisheye_fov; int reserved[3]; } Lens;
int         terra_amd_render_lens ( const TerraCamera*, const void*, HTerraScene, const TerraFramebuffer*, size_t, size_t, size_t, size_t ) __attribute__ ( ( weak ) );
int         terra_amd_render_aov_lens ( const TerraCamera*, const void*, HTerraScene, void*, size_t, size_t, size_t, size_t, size_t, size_t ) __attribute__ ( ( weak ) );
/* lightmap baking (TerraAmdPoint, TerraAmdPointSampling, TerraAmdAtlas, TerraAmdAtlasTexel and the calls of terra_amd.h "Point rendering" / "Lightmap baking",
   restated for the same reason) */
typedef struct { float position[3]; float reserved; float normal[3]; float reserved2; } BakePoint;
typedef struct { int distribution; int reserved[3]; } BakeSampling;
typedef struct { int width, height; float uv_scale[2]; float uv_offset[2]; float margin; int reserved[5]; } BakeAtlas;
typedef struct { int triangle; float wb, wc; float distance2; } BakeTexel;
int         terra_amd_atlas_points ( HTerraScene, const void*, const float*, void*, void* ) __attribute__ ( ( weak ) );
int         terra_amd_render_points ( HTerraScene, const void*, const void*, const TerraFramebuffer*, size_t, size_t, size_t, size_t ) __attribute__ ( ( weak ) );
int         terra_amd_dilate ( float*, int, int*, int, int, int ) __attribute__ ( ( weak ) );
/* probe harmonics (TerraAmdRay, TerraAmdProbeSH, TerraAmdProbeGrid and the calls of terra_amd.h "Ray-sourced rendering" / "Probe harmonics", restated for the same reason) */
typedef struct { float origin[3]; float tmax; float direction[3]; float reserved; } ProbeRay;
typedef struct { float c[9][3]; int cells; } ProbeSH;
typedef struct { float origin[3]; int nx; float spacing[3]; int ny; int nz; int reserved[3]; } ProbeGrid;
int         terra_amd_scene_vertex_points ( HTerraScene, void*, int ) __attribute__ ( ( weak ) );
int         terra_amd_probe_grid_points ( const void*, void*, int ) __attribute__ ( ( weak ) );
int         terra_amd_probe_rays ( const void*, size_t, int, const float*, void* ) __attribute__ ( ( weak ) );
int         terra_amd_render_rays ( HTerraScene, const void*, const TerraFramebuffer*, size_t, size_t, size_t, size_t ) __attribute__ ( ( weak ) );
int         terra_amd_sh_project ( const TerraFramebuffer*, const void*, size_t, int, int, void* ) __attribute__ ( ( weak ) );
/* probe visibility (TerraAmdHit, TerraAmdProbeVisibility, TerraAmdVisibilityTexel and the calls of terra_amd.h "Ray queries" / "Probe visibility", restated likewise) */
typedef struct { float t; int object; int triangle; int reserved; float point[3]; float reserved2; } ProbeHit;
typedef struct { int texels; int sharpness; float max_distance; float bias; int flags; int reserved[3]; } ProbeVisibility;
typedef struct { float weight; float distance; float distance2; int cells; } VisibilityTexel;
int         terra_amd_intersect ( HTerraScene, const void*, size_t, void* ) __attribute__ ( ( weak ) );
int         terra_amd_probe_visibility ( const void*, const void*, size_t, int, const void*, int, void* ) __attribute__ ( ( weak ) );
/* --distance-field: the records of include/terra_amd.h "Nearest-surface queries" */
typedef struct { float position[3]; float max_distance; } NearestQuery;
typedef struct { float distance; int object; unsigned triangle; unsigned feature; float point[3]; float side; } NearestAnswer;
int         terra_amd_nearest ( HTerraScene, const void*, size_t, void* ) __attribute__ ( ( weak ) );
/* --signed: the crossing counts of include/terra_amd.h "Multi-hit ray queries"; a ray is a TerraAmdRay */
typedef struct { float origin[3]; float tmax; float direction[3]; float reserved; } QueryRay;
int         terra_amd_count_hits ( HTerraScene, const void*, size_t, uint32_t* ) __attribute__ ( ( weak ) );
/* --camera-model: non-NULL = every render call and its AOV call go through the lens door */
static const Lens* g_lens = NULL;
static void render_rect ( const TerraCamera* cam, HTerraScene scene, const TerraFramebuffer* fb, size_t x, size_t y, size_t w, size_t h ) {
    if ( g_lens ) ( void ) terra_amd_render_lens ( cam, g_lens, scene, fb, x, y, w, h );
    else terra_render ( cam, scene, fb, x, y, w, h );
}
static void render_aov_rect ( const TerraCamera* cam, HTerraScene scene, void* aov, size_t W, size_t H, size_t x, size_t y, size_t w, size_t h ) {
    if ( g_lens ) ( void ) terra_amd_render_aov_lens ( cam, g_lens, scene, aov, W, H, x, y, w, h );
    else ( void ) terra_amd_render_aov ( cam, scene, aov, W, H, x, y, w, h );
}

/* ---- growable arrays ------------------------------------------------------------------------ */
#define VEC(T) struct { T* d; size_t n, cap; }
#define PUSH(v, x) do { if ( ( v ).n == ( v ).cap ) { ( v ).cap = ( v ).cap ? ( v ).cap * 2 : 256; ( v ).d = realloc ( ( v ).d, ( v ).cap * sizeof *( v ).d ); } ( v ).d[( v ).n++] = ( x ); } while ( 0 )

/* illum: Apollo's BSDF class of the material (satellite/include/Apollo.h:80-87, set ONLY by its own `illum <word>` dialect, :877-897):
   0 diffuse, 1 specular, 2 mirror, 3 pbr, 4 disney, 5 invalid = no `illum` line or a word Apollo does not know (the numeric models of
   standard MTL files included: "Unsupported material bsdf", the class stays invalid) */
enum { ILLUM_DIFFUSE = 0, ILLUM_SPECULAR, ILLUM_MIRROR, ILLUM_PBR, ILLUM_DISNEY, ILLUM_INVALID };
typedef struct { char name[128]; float kd[3], ks[3], ke[3], ns; int illum; } Mtl;
typedef struct { int v[3], t[3], n[3]; int mtl; } Face;
typedef struct { int v, t, n; } Corner;
typedef struct { size_t first, count; int group; } Poly;              /* corners [first, first + count) in file order */
typedef struct { int smooth, mtl; } Group;                            /* smooth: -1 no `s` seen, else 1 / 0 */

typedef struct {
    VEC ( TerraFloat3 ) pos, nrm;
    VEC ( TerraFloat2 ) uv;
    VEC ( Face ) faces;
    VEC ( Corner ) corners;
    VEC ( Poly ) polys;
    VEC ( Group ) groups;
    VEC ( Mtl ) mtls;
} Model;

static int find_mtl ( Model* m, const char* name ) {
    for ( size_t i = 0; i < m->mtls.n; ++i ) if ( strcmp ( m->mtls.d[i].name, name ) == 0 ) return ( int ) i;
    return -1;
}

static void load_mtl ( Model* m, const char* dir, const char* file ) {
    char path[2048];
    snprintf ( path, sizeof path, "%s%s", dir, file );
    FILE* f = fopen ( path, "r" );
    if ( !f ) { fprintf ( stderr, "terra_headless: cannot open material library %s\n", path ); return; }
    char line[1024]; Mtl* cur = NULL;
    while ( fgets ( line, sizeof line, f ) ) {
        char key[64]; int off = 0;
        if ( sscanf ( line, "%63s%n", key, &off ) != 1 || key[0] == '#' ) continue;
        const char* rest = line + off;
        if ( strcmp ( key, "newmtl" ) == 0 ) {
            Mtl x; memset ( &x, 0, sizeof x );
            sscanf ( rest, "%127s", x.name );
            x.kd[0] = x.kd[1] = x.kd[2] = 0.7f; x.ns = 1.f; x.illum = ILLUM_INVALID;
            PUSH ( m->mtls, x ); cur = &m->mtls.d[m->mtls.n - 1];
        } else if ( cur ) {
            if ( strcmp ( key, "Kd" ) == 0 ) sscanf ( rest, "%f %f %f", &cur->kd[0], &cur->kd[1], &cur->kd[2] );
            else if ( strcmp ( key, "Ks" ) == 0 ) sscanf ( rest, "%f %f %f", &cur->ks[0], &cur->ks[1], &cur->ks[2] );
            else if ( strcmp ( key, "Ke" ) == 0 ) sscanf ( rest, "%f %f %f", &cur->ke[0], &cur->ke[1], &cur->ke[2] );
            else if ( strcmp ( key, "Ns" ) == 0 ) sscanf ( rest, "%f", &cur->ns );
            else if ( strcmp ( key, "illum" ) == 0 ) {
                static const char* words[] = { "diffuse", "specular", "mirror", "pbr", "disney" };
                char v[64] = ""; sscanf ( rest, "%63s", v );
                for ( int k = 0; k < 5; ++k ) if ( !strcmp ( v, words[k] ) ) cur->illum = k;      /* any other word leaves the class as it was (Apollo.h:895-897) */
            }
        }
    }
    fclose ( f );
}

static int fix_index ( int i, size_t n ) { return i > 0 ? i - 1 : ( i < 0 ? ( int ) n + i : -1 ); }

static int load_obj ( Model* m, const char* path ) {
    FILE* f = fopen ( path, "r" );
    if ( !f ) { fprintf ( stderr, "terra_headless: cannot open %s\n", path ); return 0; }
    char dir[1024] = "";
    const char* slash = strrchr ( path, '/' );
    if ( slash ) { size_t k = ( size_t ) ( slash - path ) + 1; if ( k < sizeof dir ) { memcpy ( dir, path, k ); dir[k] = 0; } }
    char line[4096]; int cur_mtl = -1;
#define NEED_GROUP() do { if ( m->groups.n == 0 ) { Group g0 = { -1, -1 }; PUSH ( m->groups, g0 ); } } while ( 0 )
    while ( fgets ( line, sizeof line, f ) ) {
        char* p = line;
        while ( isspace ( ( unsigned char ) *p ) ) ++p;
        if ( p[0] == 'v' && p[1] == ' ' ) { TerraFloat3 v = { 0, 0, 0 }; sscanf ( p + 2, "%f %f %f", &v.x, &v.y, &v.z ); PUSH ( m->pos, v ); }
        else if ( p[0] == 'v' && p[1] == 'n' ) { TerraFloat3 v = { 0, 0, 0 }; sscanf ( p + 3, "%f %f %f", &v.x, &v.y, &v.z ); PUSH ( m->nrm, v ); }
        else if ( p[0] == 'v' && p[1] == 't' ) { TerraFloat2 v = { 0, 0 }; sscanf ( p + 3, "%f %f", &v.x, &v.y ); PUSH ( m->uv, v ); }
        else if ( p[0] == 'f' && isspace ( ( unsigned char ) p[1] ) ) {
            int vi[64], ti[64], ni[64], cnt = 0;
            char* tok = strtok ( p + 2, " \t\r\n" );
            while ( tok && cnt < 64 ) {
                int a = 0, b = 0, c = 0;
                if ( sscanf ( tok, "%d/%d/%d", &a, &b, &c ) == 3 ) {}
                else if ( sscanf ( tok, "%d//%d", &a, &c ) == 2 ) { b = 0; }
                else if ( sscanf ( tok, "%d/%d", &a, &b ) == 2 ) { c = 0; }
                else { sscanf ( tok, "%d", &a ); b = c = 0; }
                vi[cnt] = fix_index ( a, m->pos.n ); ti[cnt] = fix_index ( b, m->uv.n ); ni[cnt] = fix_index ( c, m->nrm.n ); ++cnt;
                tok = strtok ( NULL, " \t\r\n" );
            }
            if ( cnt >= 3 ) {
                NEED_GROUP();
                Poly pl = { m->corners.n, ( size_t ) cnt, ( int ) m->groups.n - 1 };
                int ok = 1;
                for ( int k = 0; k < cnt; ++k ) if ( vi[k] < 0 ) ok = 0;
                if ( ok ) { for ( int k = 0; k < cnt; ++k ) { Corner c = { vi[k], ti[k], ni[k] }; PUSH ( m->corners, c ); } PUSH ( m->polys, pl ); }
            }
            for ( int k = 1; k + 1 < cnt; ++k ) {       /* fan triangulation */
                Face fc = { { vi[0], vi[k], vi[k + 1] }, { ti[0], ti[k], ti[k + 1] }, { ni[0], ni[k], ni[k + 1] }, cur_mtl };
                if ( fc.v[0] >= 0 && fc.v[1] >= 0 && fc.v[2] >= 0 ) PUSH ( m->faces, fc );
            }
        } else if ( strncmp ( p, "usemtl", 6 ) == 0 ) { char name[128] = ""; sscanf ( p + 6, "%127s", name ); cur_mtl = find_mtl ( m, name ); NEED_GROUP(); m->groups.d[m->groups.n - 1].mtl = cur_mtl; }
        else if ( ( p[0] == 'g' || p[0] == 'o' ) && p[1] == ' ' ) { Group g = { -1, -1 }; PUSH ( m->groups, g ); }       /* Apollo.h:1205-1218: groups and objects alike open a mesh */
        else if ( p[0] == 's' && p[1] == ' ' ) { NEED_GROUP(); m->groups.d[m->groups.n - 1].smooth = p[2] == '1' ? 1 : 0; }           /* Apollo.h:1225-1240: smooth iff the character after "s " is '1' */
        else if ( strncmp ( p, "mtllib", 6 ) == 0 ) { char name[512] = ""; sscanf ( p + 6, "%511s", name ); load_mtl ( m, dir, name ); }
    }
    fclose ( f );
    return m->faces.n > 0;
}

/* ---- scene construction ---------------------------------------------------------------------- */
static TerraFloat3 flipz ( TerraFloat3 v, int flip ) { if ( flip ) v.z = -v.z; return v; }

static void set_material ( TerraObject* o, const Mtl* mt, int apollo );
static void dump_object ( FILE* f, size_t j, const TerraObject* o );

static HTerraScene build_scene ( Model* m, int flip, FILE* dump ) {
    /* smooth normals per position for faces without vn */
    TerraFloat3* smooth = calloc ( m->pos.n ? m->pos.n : 1, sizeof ( TerraFloat3 ) );
    for ( size_t i = 0; i < m->faces.n; ++i ) {
        Face* f = &m->faces.d[i];
        TerraFloat3 a = m->pos.d[f->v[0]], b = m->pos.d[f->v[1]], c = m->pos.d[f->v[2]];
        TerraFloat3 e1 = terra_subf3 ( &b, &a ), e2 = terra_subf3 ( &c, &a ), n = terra_crossf3 ( &e1, &e2 );   /* area weighted */
        for ( int k = 0; k < 3; ++k ) smooth[f->v[k]] = terra_addf3 ( &smooth[f->v[k]], &n );
    }
    HTerraScene scene = terra_scene_create();
    int groups = ( int ) m->mtls.n + 1;                      /* one object per material; the last holds faces without one */
    for ( int g = 0; g < groups; ++g ) {
        int want = g < ( int ) m->mtls.n ? g : -1;
        size_t cnt = 0;
        for ( size_t i = 0; i < m->faces.n; ++i ) if ( m->faces.d[i].mtl == want ) ++cnt;
        if ( !cnt ) continue;
        TerraObject* o = terra_scene_add_object ( scene, cnt );
        size_t k = 0;
        for ( size_t i = 0; i < m->faces.n; ++i ) {
            Face* f = &m->faces.d[i];
            if ( f->mtl != want ) continue;
            /* flipping z mirrors the mesh; swapping b and c restores the winding (Scene.cpp:90-93) */
            int order[3] = { 0, flip ? 2 : 1, flip ? 1 : 2 };
            TerraFloat3 P[3], N[3]; TerraFloat2 T[3];
            for ( int c = 0; c < 3; ++c ) {
                int s = order[c];
                P[c] = flipz ( m->pos.d[f->v[s]], flip );
                TerraFloat3 n = f->n[s] >= 0 ? m->nrm.d[f->n[s]] : smooth[f->v[s]];
                float len = terra_lenf3 ( &n );
                N[c] = len > 0.f ? terra_normf3 ( &n ) : terra_f3_set ( 0.f, 1.f, 0.f );
                N[c] = flipz ( N[c], flip );
                T[c] = f->t[s] >= 0 ? m->uv.d[f->t[s]] : terra_f2_set ( 0.f, 0.f );
            }
            o->triangles[k].a = P[0]; o->triangles[k].b = P[1]; o->triangles[k].c = P[2];
            o->properties[k].normal_a = N[0]; o->properties[k].normal_b = N[1]; o->properties[k].normal_c = N[2];
            o->properties[k].texcoord_a = T[0]; o->properties[k].texcoord_b = T[1]; o->properties[k].texcoord_c = T[2];
            ++k;
        }
        Mtl def; memset ( &def, 0, sizeof def ); def.kd[0] = def.kd[1] = def.kd[2] = 0.7f; def.ns = 1.f; def.illum = ILLUM_INVALID;
        set_material ( o, want >= 0 ? &m->mtls.d[want] : &def, 0 );
        if ( dump ) dump_object ( dump, terra_scene_count_objects ( scene ) - 1, o );
    }
    free ( smooth );
    return scene;
}

/* ---- the reference importer's policy (see the header comment) ------------------------------------ */
typedef struct { TerraFloat3 pos; TerraFloat2 tex; TerraFloat3 norm; VEC ( unsigned ) adj; } AVert;
typedef struct { unsigned bits[3]; unsigned value; int used; } VSlot;
static unsigned pos_hash ( const unsigned* b ) { unsigned h = 2166136261u; for ( int i = 0; i < 3; ++i ) { h ^= b[i]; h *= 16777619u; h ^= h >> 13; } return h; }

/* Material class -> preset. apollo = 1: the reference client's switch (satellite/src/Scene.cpp:193-230): APOLLO_SPECULAR -> Phong; mirror, pbr and
   everything else (disney, and the invalid class of a material without an Apollo `illum` word) fall through its warnings to diffuse.
   apollo = 0 (--normals file, this repo's policy for standard MTL files): `illum specular`, or no Apollo word and Ks > 0, -> Phong. */
static void set_material ( TerraObject* o, const Mtl* mt, int apollo ) {
    TerraFloat3 kd = terra_f3_setv ( mt->kd ), ks = terra_f3_setv ( mt->ks ), ke = terra_f3_setv ( mt->ke ), zero = terra_f3_zero;
    o->material.ior = 1.5f;                                /* Scene.cpp:187 */
    terra_attribute_init_constant ( &o->material.emissive, &ke );
    int phong = mt->illum == ILLUM_SPECULAR;
    if ( !apollo && mt->illum == ILLUM_INVALID ) phong = ks.x + ks.y + ks.z > 0.f;
    if ( apollo && mt->illum != ILLUM_SPECULAR && mt->illum != ILLUM_DIFFUSE ) {      /* the reference warns and goes on (Scene.cpp:215-220) */
        static const char* what[] = { "", "", "mirror", "pbr", "disney", "unclassified (no Apollo `illum` word)" };
        fprintf ( stderr, "terra_headless: unsupported %s material(%s). Defaulting to diffuse\n", what[mt->illum], mt->name[0] ? mt->name : "<none>" );
    }
    if ( phong ) {                                         /* specular -> Phong (Scene.cpp:193-213) */
        TerraFloat3 ns = terra_f3_set1 ( mt->ns );
        terra_attribute_init_constant ( &o->material.attributes[TERRA_PHONG_ALBEDO], &kd );
        terra_attribute_init_constant ( &o->material.attributes[TERRA_PHONG_SPECULAR_COLOR], &ks );
        terra_attribute_init_constant ( &o->material.attributes[TERRA_PHONG_SPECULAR_INTENSITY], &ns );
        terra_attribute_init_constant ( &o->material.attributes[TERRA_PHONG_SAMPLE_PICK], &zero );
        o->material.attributes_count = TERRA_PHONG_END;
        terra_bsdf_phong_init ( &o->material.bsdf );
    } else {                                               /* everything else -> diffuse (Scene.cpp:215-230) */
        terra_attribute_init_constant ( &o->material.attributes[TERRA_DIFFUSE_ALBEDO], &kd );
        o->material.attributes_count = TERRA_DIFFUSE_END;
        terra_bsdf_diffuse_init ( &o->material.bsdf );
    }
}

static HTerraScene build_scene_apollo ( Model* m, int flip, FILE* dump ) {
    VEC ( AVert ) verts; memset ( &verts, 0, sizeof verts );
    VEC ( unsigned ) idx; memset ( &idx, 0, sizeof idx );
    VEC ( int ) tri_group; memset ( &tri_group, 0, sizeof tri_group );
    size_t cap = 64; while ( cap < 4 * ( m->corners.n + 1 ) ) cap *= 2;
    VSlot* table = calloc ( cap, sizeof ( VSlot ) );
    int zero_used = 0; unsigned zero_value = 0;
    unsigned face_count = 0;
    for ( size_t pi = 0; pi < m->polys.n; ++pi ) {
        const Poly* pl = &m->polys.d[pi];
        const int smooth = m->groups.d[pl->group].smooth;
        unsigned first = 0, last = 0;
        for ( size_t j = 0; j < pl->count; ++j ) {
            const Corner* c = &m->corners.d[pl->first + j];
            TerraFloat3 pos = flipz ( m->pos.d[c->v], flip );                     /* z is negated when the `v` line is read (Apollo.h:1167) */
            unsigned bits[3]; memcpy ( bits, &pos, 12 );
            for ( int k = 0; k < 3; ++k ) if ( bits[k] == 0x80000000u ) bits[k] = 0;      /* float equality: -0 == +0 */
            const int is_zero = !bits[0] && !bits[1] && !bits[2];
            unsigned index = 0; int dup = 0;
            size_t slot = pos_hash ( bits ) & ( cap - 1 );
            if ( smooth == 1 ) {                                                  /* lookup only inside smooth groups (Apollo.h:1349-1356) */
                if ( is_zero ) { if ( zero_used ) { index = zero_value; dup = 1; } }
                else for ( size_t s2 = slot; table[s2].used; s2 = ( s2 + 1 ) & ( cap - 1 ) ) if ( !memcmp ( table[s2].bits, bits, 12 ) ) { index = table[s2].value; dup = 1; break; }      /* the first one inserted */
            }
            if ( !dup ) {
                AVert v; memset ( &v, 0, sizeof v );
                v.pos = pos; v.tex = c->t >= 0 ? m->uv.d[c->t] : terra_f2_set ( 0.f, 0.f );
                PUSH ( verts, v ); index = ( unsigned ) verts.n - 1;
                if ( is_zero ) { zero_used = 1; zero_value = index; }              /* the all-zero key keeps the LAST vertex (Apollo.h:2180-2184) */
                else { size_t s2 = slot; while ( table[s2].used ) s2 = ( s2 + 1 ) & ( cap - 1 ); memcpy ( table[s2].bits, bits, 12 ); table[s2].value = index; table[s2].used = 1; }
            }
            {   /* adjacency: the triangle being formed while this corner is parsed (Apollo.h:1373-1381) */
                AVert* v = &verts.d[index]; int seen = 0;
                for ( size_t a = 0; a < v->adj.n; ++a ) if ( v->adj.d[a] == face_count ) seen = 1;
                if ( !seen ) PUSH ( v->adj, face_count );
            }
            if ( j == 0 ) first = index;
            if ( j >= 3 ) { PUSH ( idx, first ); PUSH ( idx, last ); }             /* fan: (first, previous, current) */
            PUSH ( idx, index );
            if ( j >= 2 ) { last = index; PUSH ( tri_group, pl->group ); ++face_count; }
        }
    }
    if ( flip ) for ( size_t i = 0; i + 2 < idx.n; i += 3 ) { unsigned t = idx.d[i]; idx.d[i] = idx.d[i + 2]; idx.d[i + 2] = t; }      /* Apollo.h:1412-1418 */
    TerraFloat3* fn = malloc ( ( face_count ? face_count : 1 ) * sizeof ( TerraFloat3 ) );
    for ( unsigned i = 0; i < face_count; ++i ) {                                  /* Apollo.h:1438-1462 */
        TerraFloat3 v0 = verts.d[idx.d[3 * i]].pos, v1 = verts.d[idx.d[3 * i + 1]].pos, v2 = verts.d[idx.d[3 * i + 2]].pos;
        TerraFloat3 e01 = { v1.x - v0.x, v1.y - v0.y, v1.z - v0.z }, e02 = { v2.x - v0.x, v2.y - v0.y, v2.z - v0.z };
        TerraFloat3 n = { e01.y * e02.z - e01.z * e02.y, e01.z * e02.x - e01.x * e02.z, e01.x * e02.y - e01.y * e02.x };
        float len = sqrtf ( n.x * n.x + n.y * n.y + n.z * n.z );
        n.x /= len; n.y /= len; n.z /= len;
        fn[i] = n;
    }
    unsigned char* done = calloc ( verts.n ? verts.n : 1, 1 );
    for ( size_t g = 0; g < m->groups.n; ++g ) {                                   /* Apollo.h:1465-1541, group after group */
        memset ( done, 0, verts.n );
        for ( unsigned i = 0; i < face_count; ++i ) {
            if ( tri_group.d[i] != ( int ) g ) continue;
            for ( int k = 0; k < 3; ++k ) {
                AVert* v = &verts.d[idx.d[3 * i + k]];
                if ( m->groups.d[g].smooth == 0 ) { v->norm = fn[i]; continue; }
                if ( done[idx.d[3 * i + k]] ) continue;
                done[idx.d[3 * i + k]] = 1;
                TerraFloat3 sum = { 0.f, 0.f, 0.f };
                for ( size_t a = 0; a < v->adj.n; ++a ) { sum.x += fn[v->adj.d[a]].x; sum.y += fn[v->adj.d[a]].y; sum.z += fn[v->adj.d[a]].z; }
                float len = sqrtf ( sum.x * sum.x + sum.y * sum.y + sum.z * sum.z );
                sum.x /= len; sum.y /= len; sum.z /= len;
                v->norm = sum;
            }
        }
    }
    HTerraScene scene = terra_scene_create();
    for ( size_t g = 0; g < m->groups.n; ++g ) {
        size_t cnt = 0;
        for ( unsigned i = 0; i < face_count; ++i ) if ( tri_group.d[i] == ( int ) g ) ++cnt;
        if ( !cnt ) continue;
        TerraObject* o = terra_scene_add_object ( scene, cnt );
        size_t k = 0;
        for ( unsigned i = 0; i < face_count; ++i ) {
            if ( tri_group.d[i] != ( int ) g ) continue;
            const AVert* a = &verts.d[idx.d[3 * i]]; const AVert* b = &verts.d[idx.d[3 * i + 1]]; const AVert* c = &verts.d[idx.d[3 * i + 2]];
            o->triangles[k].a = a->pos; o->triangles[k].b = b->pos; o->triangles[k].c = c->pos;
            o->properties[k].normal_a = a->norm; o->properties[k].normal_b = b->norm; o->properties[k].normal_c = c->norm;
            o->properties[k].texcoord_a = a->tex; o->properties[k].texcoord_b = b->tex; o->properties[k].texcoord_c = c->tex;
            ++k;
        }
        Mtl def; memset ( &def, 0, sizeof def ); def.kd[0] = def.kd[1] = def.kd[2] = 0.7f; def.ns = 1.f; def.illum = ILLUM_INVALID;
        set_material ( o, m->groups.d[g].mtl >= 0 ? &m->mtls.d[m->groups.d[g].mtl] : &def, 1 );
        if ( dump ) dump_object ( dump, terra_scene_count_objects ( scene ) - 1, o );
    }
    for ( size_t i = 0; i < verts.n; ++i ) free ( verts.d[i].adj.d );
    free ( verts.d ); free ( idx.d ); free ( tri_group.d ); free ( table ); free ( fn ); free ( done );
    return scene;
}

/* --dump-scene: every object exactly as it was filled through terra_scene_add_object (text, %.9g round-trips a float): for the loader's tests */
static void dump_object ( FILE* f, size_t j, const TerraObject* o ) {
    fprintf ( f, "object %zu triangles %zu attributes %zu\n", j, o->triangles_count, o->material.attributes_count );
    {   /* the material as it was filled: preset (by its attribute count), constant attribute values in slot order, emissive, ior */
        const TerraMaterial* mt = &o->material;
        fprintf ( f, "m %s", mt->attributes_count == TERRA_PHONG_END ? "phong" : "diffuse" );
        for ( size_t a = 0; a < mt->attributes_count; ++a ) fprintf ( f, " %.9g %.9g %.9g", mt->attributes[a].value.x, mt->attributes[a].value.y, mt->attributes[a].value.z );
        fprintf ( f, " e %.9g %.9g %.9g ior %.9g\n", mt->emissive.value.x, mt->emissive.value.y, mt->emissive.value.z, mt->ior );
    }
    for ( size_t i = 0; i < o->triangles_count; ++i ) {
        const TerraTriangle* t = &o->triangles[i]; const TerraTriangleProperties* q = &o->properties[i];
        fprintf ( f, "t %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g n %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g uv %.9g %.9g %.9g %.9g %.9g %.9g\n",
                  t->a.x, t->a.y, t->a.z, t->b.x, t->b.y, t->b.z, t->c.x, t->c.y, t->c.z,
                  q->normal_a.x, q->normal_a.y, q->normal_a.z, q->normal_b.x, q->normal_b.y, q->normal_b.z, q->normal_c.x, q->normal_c.y, q->normal_c.z,
                  q->texcoord_a.x, q->texcoord_a.y, q->texcoord_b.x, q->texcoord_b.y, q->texcoord_c.x, q->texcoord_c.y );
    }
}

/* ---- image writers --------------------------------------------------------------------------- */
static unsigned char to_byte ( float v ) { v = v < 0.f ? 0.f : ( v > 1.f ? 1.f : v ); return ( unsigned char ) ( v * 255.f ); }   /* Visualization.cpp:331-338 */

static int write_ppm ( const char* path, const TerraFramebuffer* fb ) {
    FILE* f = fopen ( path, "wb" ); if ( !f ) return 0;
    fprintf ( f, "P6\n%zu %zu\n255\n", fb->width, fb->height );
    for ( size_t i = 0; i < fb->width * fb->height; ++i ) { unsigned char px[3] = { to_byte ( fb->pixels[i].x ), to_byte ( fb->pixels[i].y ), to_byte ( fb->pixels[i].z ) }; fwrite ( px, 1, 3, f ); }
    return fclose ( f ) == 0;
}
static int write_pfm ( const char* path, const TerraFramebuffer* fb ) {
    FILE* f = fopen ( path, "wb" ); if ( !f ) return 0;
    fprintf ( f, "PF\n%zu %zu\n-1.0\n", fb->width, fb->height );
    for ( size_t y = fb->height; y-- > 0; ) fwrite ( &fb->pixels[y * fb->width], sizeof ( TerraFloat3 ), fb->width, f );   /* bottom row first */
    return fclose ( f ) == 0;
}
/* the means over hits of one AOV (k: 0 albedo, 1 normal, 2 depth) as a PFM; pixels no sample hit are 0 */
static int write_aov_pfm ( const char* path, const AovSum* a, size_t W, size_t H, int k ) {
    TerraFramebuffer img; img.width = W; img.height = H; img.results = NULL;
    img.pixels = malloc ( W * H * sizeof ( TerraFloat3 ) );
    if ( !img.pixels ) return 0;
    for ( size_t i = 0; i < W * H; ++i ) {
        const float c = a[i].coverage;
        float v[3] = { 0.f, 0.f, 0.f };
        if ( c > 0.f ) for ( int ch = 0; ch < 3; ++ch ) v[ch] = ( k == 0 ? a[i].albedo[ch] : k == 1 ? a[i].normal[ch] : a[i].depth ) / c;
        img.pixels[i] = terra_f3_set ( v[0], v[1], v[2] );
    }
    const int ok = write_pfm ( path, &img );
    free ( img.pixels );
    return ok;
}
/* the variance of each pixel's mean luminance (m2 / (weight (batches - 1))) as a grey PFM; pixels with fewer than two batches are 0 */
static int write_variance_pfm ( const char* path, const MomentSum* m, size_t W, size_t H ) {
    TerraFramebuffer img; img.width = W; img.height = H; img.results = NULL;
    img.pixels = malloc ( W * H * sizeof ( TerraFloat3 ) );
    if ( !img.pixels ) return 0;
    for ( size_t i = 0; i < W * H; ++i ) {
        const float v = m[i].batches >= 2 ? m[i].m2 / ( ( float ) m[i].weight * ( float ) ( m[i].batches - 1 ) ) : 0.f;
        img.pixels[i] = terra_f3_set ( v, v, v );
    }
    const int ok = write_pfm ( path, &img );
    free ( img.pixels );
    return ok;
}
static int write_hdr ( const char* path, const TerraFramebuffer* fb ) {       /* Radiance RGBE, flat scanlines */
    FILE* f = fopen ( path, "wb" ); if ( !f ) return 0;
    fprintf ( f, "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %zu +X %zu\n", fb->height, fb->width );
    for ( size_t i = 0; i < fb->width * fb->height; ++i ) {
        float r = fb->pixels[i].x, g = fb->pixels[i].y, b = fb->pixels[i].z, mx = r > g ? ( r > b ? r : b ) : ( g > b ? g : b );
        unsigned char px[4] = { 0, 0, 0, 0 };
        if ( mx > 1e-32f ) { int e; float s = frexpf ( mx, &e ) * 256.f / mx; px[0] = ( unsigned char ) ( r * s ); px[1] = ( unsigned char ) ( g * s ); px[2] = ( unsigned char ) ( b * s ); px[3] = ( unsigned char ) ( e + 128 ); }
        fwrite ( px, 1, 4, f );
    }
    return fclose ( f ) == 0;
}
/* PNG with stored (uncompressed) deflate blocks: valid everywhere, no zlib needed */
static unsigned long crc_table[256];
static unsigned long crc32_of ( unsigned long c, const unsigned char* p, size_t n ) {
    if ( !crc_table[1] ) for ( unsigned long i = 0; i < 256; ++i ) { unsigned long k = i; for ( int j = 0; j < 8; ++j ) k = k & 1 ? 0xedb88320ul ^ ( k >> 1 ) : k >> 1; crc_table[i] = k; }
    c ^= 0xfffffffful;
    for ( size_t i = 0; i < n; ++i ) c = crc_table[ ( c ^ p[i] ) & 0xff] ^ ( c >> 8 );
    return c ^ 0xfffffffful;
}
static void be32 ( unsigned char* p, unsigned long v ) { p[0] = ( unsigned char ) ( v >> 24 ); p[1] = ( unsigned char ) ( v >> 16 ); p[2] = ( unsigned char ) ( v >> 8 ); p[3] = ( unsigned char ) v; }
static void png_chunk ( FILE* f, const char* type, const unsigned char* data, size_t n ) {
    unsigned char hdr[8]; be32 ( hdr, ( unsigned long ) n ); memcpy ( hdr + 4, type, 4 ); fwrite ( hdr, 1, 8, f );
    if ( n ) fwrite ( data, 1, n, f );
    unsigned char* tmp = malloc ( n + 4 ); memcpy ( tmp, type, 4 ); if ( n ) memcpy ( tmp + 4, data, n );
    unsigned long c = crc32_of ( 0, tmp, n + 4 ); free ( tmp );       /* CRC covers type + data */
    unsigned char tail[4]; be32 ( tail, c ); fwrite ( tail, 1, 4, f );
}
static int write_png ( const char* path, const TerraFramebuffer* fb ) {
    FILE* f = fopen ( path, "wb" ); if ( !f ) return 0;
    const size_t W = fb->width, H = fb->height, row = 1 + 3 * W, raw_n = row * H;
    unsigned char* raw = malloc ( raw_n );
    for ( size_t y = 0; y < H; ++y ) {
        raw[y * row] = 0;       /* filter: none */
        for ( size_t x = 0; x < W; ++x ) { const TerraFloat3* p = &fb->pixels[y * W + x]; unsigned char* q = raw + y * row + 1 + 3 * x; q[0] = to_byte ( p->x ); q[1] = to_byte ( p->y ); q[2] = to_byte ( p->z ); }
    }
    size_t blocks = ( raw_n + 65534 ) / 65535, zn = 2 + raw_n + 5 * blocks + 4;
    unsigned char* z = malloc ( zn ); size_t o = 0;
    z[o++] = 0x78; z[o++] = 0x01;
    unsigned long a = 1, b = 0;
    for ( size_t i = 0; i < raw_n; ++i ) { a = ( a + raw[i] ) % 65521; b = ( b + a ) % 65521; }
    for ( size_t off = 0; off < raw_n; off += 65535 ) {
        size_t n = raw_n - off < 65535 ? raw_n - off : 65535;
        z[o++] = off + n == raw_n ? 1 : 0; z[o++] = ( unsigned char ) ( n & 0xff ); z[o++] = ( unsigned char ) ( n >> 8 ); z[o++] = ( unsigned char ) ( ~n & 0xff ); z[o++] = ( unsigned char ) ( ( ~n >> 8 ) & 0xff );
        memcpy ( z + o, raw + off, n ); o += n;
    }
    be32 ( z + o, ( b << 16 ) | a ); o += 4;
    static const unsigned char sig[8] = { 0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a };
    fwrite ( sig, 1, 8, f );
    unsigned char ihdr[13]; be32 ( ihdr, ( unsigned long ) W ); be32 ( ihdr + 4, ( unsigned long ) H ); ihdr[8] = 8; ihdr[9] = 2; ihdr[10] = ihdr[11] = ihdr[12] = 0;
    png_chunk ( f, "IHDR", ihdr, 13 ); png_chunk ( f, "IDAT", z, o ); png_chunk ( f, "IEND", NULL, 0 );
    free ( raw ); free ( z );
    return fclose ( f ) == 0;
}
/* A grid of counts[a] cells per axis over the bounding box of nv > 0 vertices (--bake-probes, --distance-field): lo = the box's lower corner, sp = the cell size -- 1 on
   an axis the scene has no extent on --; returns the squared diagonal of the box */
static double cell_grid_over ( const BakePoint* verts, int nv, const int counts[3], float lo[3], float sp[3] ) {
    double diagonal2 = 0.;
    for ( int a = 0; a < 3; ++a ) {
        float hi = lo[a] = verts[0].position[a];
        for ( int k = 1; k < nv; ++k ) { const float v = verts[k].position[a]; if ( v < lo[a] ) lo[a] = v; if ( v > hi ) hi = v; }
        diagonal2 += ( double ) ( hi - lo[a] ) * ( double ) ( hi - lo[a] );
        sp[a] = ( hi - lo[a] ) / ( float ) counts[a];
        if ( !( sp[a] > 0.f ) ) sp[a] = 1.f;
    }
    return diagonal2;
}
static int write_image ( const char* path, const TerraFramebuffer* fb ) {
    const char* ext = strrchr ( path, '.' );
    if ( ext && strcmp ( ext, ".ppm" ) == 0 ) return write_ppm ( path, fb );
    if ( ext && strcmp ( ext, ".pfm" ) == 0 ) return write_pfm ( path, fb );
    if ( ext && strcmp ( ext, ".hdr" ) == 0 ) return write_hdr ( path, fb );
    return write_png ( path, fb );      /* png assumed by default, as Visualization.cpp:313-316 */
}

/* ---- environment maps in ----------------------------------------------------------------------- */
/* A lat-long map as W x H x 3 floats, row 0 = the top (+y) row, the order the lat-long lookup reads. Returns NULL with `err` set; the caller exits 65. */
static float* map_fail ( char* err, size_t n, const char* msg, FILE* f, float* px ) { snprintf ( err, n, "%s", msg ); if ( f ) fclose ( f ); free ( px ); return NULL; }
static int read_line ( FILE* f, char* buf, size_t n ) {            /* one header line without its newline; 0 at end of file */
    size_t k = 0; int c;
    while ( ( c = fgetc ( f ) ) != EOF && c != '\n' ) if ( k + 1 < n ) buf[k++] = ( char ) c;
    buf[k] = 0;
    return c != EOF || k > 0;
}
static float* load_hdr ( const char* path, size_t* W, size_t* H, char* err, size_t en ) {
    FILE* f = fopen ( path, "rb" ); if ( !f ) return map_fail ( err, en, "cannot open", NULL, NULL );
    char line[512];
    if ( !read_line ( f, line, sizeof line ) || strncmp ( line, "#?", 2 ) ) return map_fail ( err, en, "not a Radiance file (no #? signature)", f, NULL );
    for ( ;; ) {                                                    /* header lines up to the blank one */
        if ( !read_line ( f, line, sizeof line ) ) return map_fail ( err, en, "truncated header", f, NULL );
        if ( !line[0] ) break;
        if ( !strncmp ( line, "FORMAT=", 7 ) && strcmp ( line + 7, "32-bit_rle_rgbe" ) ) return map_fail ( err, en, "unsupported FORMAT (only 32-bit_rle_rgbe)", f, NULL );
    }
    long h = 0, w = 0; char tail;
    if ( !read_line ( f, line, sizeof line ) || sscanf ( line, "-Y %ld +X %ld %c", &h, &w, &tail ) != 2 ) return map_fail ( err, en, "unsupported orientation (only -Y H +X W)", f, NULL );
    if ( w < 1 || h < 1 || w > 65535 || h > 65535 ) return map_fail ( err, en, "size out of range (1 .. 65535 per dimension)", f, NULL );
    float* px = malloc ( ( size_t ) w * h * 3 * sizeof ( float ) );
    unsigned char* row = malloc ( ( size_t ) w * 4 );
    if ( !px || !row ) { free ( row ); return map_fail ( err, en, "out of memory for the map", f, px ); }
    for ( long y = 0; y < h; ++y ) {
        unsigned char q[4];
        if ( fread ( q, 1, 4, f ) != 4 ) { free ( row ); return map_fail ( err, en, "truncated pixel data", f, px ); }
        if ( w >= 8 && w <= 0x7fff && q[0] == 2 && q[1] == 2 && ( ( q[2] << 8 ) | q[3] ) == w ) {      /* new-style RLE: the four channels one after the other */
            for ( int ch = 0; ch < 4; ++ch ) {
                for ( long x = 0; x < w; ) {
                    int c = fgetc ( f ), run;
                    if ( c == EOF || c == 0 ) { free ( row ); return map_fail ( err, en, c == EOF ? "truncated pixel data" : "bad run length", f, px ); }
                    run = c > 128 ? c - 128 : c;
                    if ( x + run > w ) { free ( row ); return map_fail ( err, en, "run past the end of a scanline", f, px ); }
                    if ( c > 128 ) { int v = fgetc ( f ); if ( v == EOF ) { free ( row ); return map_fail ( err, en, "truncated pixel data", f, px ); } for ( int k = 0; k < run; ++k ) row[4 * ( x + k ) + ch] = ( unsigned char ) v; }
                    else for ( int k = 0; k < run; ++k ) { int v = fgetc ( f ); if ( v == EOF ) { free ( row ); return map_fail ( err, en, "truncated pixel data", f, px ); } row[4 * ( x + k ) + ch] = ( unsigned char ) v; }
                    x += run;
                }
            }
        } else {                                                    /* flat: q is the first texel */
            memcpy ( row, q, 4 );
            if ( w > 1 && fread ( row + 4, 4, ( size_t ) w - 1, f ) != ( size_t ) w - 1 ) { free ( row ); return map_fail ( err, en, "truncated pixel data", f, px ); }
        }
        for ( long x = 0; x < w; ++x ) {
            const unsigned char* t = row + 4 * x; float* o = px + ( ( size_t ) y * w + x ) * 3;
            for ( int ch = 0; ch < 3; ++ch ) o[ch] = t[3] ? ldexpf ( ( float ) t[ch], ( int ) t[3] - 136 ) : 0.f;
        }
    }
    free ( row ); fclose ( f );
    *W = ( size_t ) w; *H = ( size_t ) h;
    return px;
}
static float* load_pfm ( const char* path, size_t* W, size_t* H, char* err, size_t en ) {
    FILE* f = fopen ( path, "rb" ); if ( !f ) return map_fail ( err, en, "cannot open", NULL, NULL );
    char magic[3] = { 0 }; long w = 0, h = 0; double scale = 0.;
    if ( fscanf ( f, "%2s %ld %ld %lf", magic, &w, &h, &scale ) != 4 || strcmp ( magic, "PF" ) || scale == 0. ) return map_fail ( err, en, "not a colour PFM (PF W H scale)", f, NULL );
    if ( fgetc ( f ) == EOF ) return map_fail ( err, en, "truncated header", f, NULL );     /* the single whitespace byte before the data */
    if ( w < 1 || h < 1 || w > 65535 || h > 65535 ) return map_fail ( err, en, "size out of range (1 .. 65535 per dimension)", f, NULL );
    const size_t n = ( size_t ) w * h * 3;
    float* px = malloc ( n * sizeof ( float ) );
    if ( !px ) return map_fail ( err, en, "out of memory for the map", f, NULL );
    const uint16_t probe = 1; const int host_le = *( const uint8_t* ) &probe == 1, file_le = scale < 0.;
    for ( long y = h; y-- > 0; ) {                                  /* bottom row first in the file */
        float* o = px + ( size_t ) y * w * 3;
        if ( fread ( o, sizeof ( float ), ( size_t ) w * 3, f ) != ( size_t ) w * 3 ) return map_fail ( err, en, "truncated pixel data", f, px );
        if ( host_le != file_le ) for ( long k = 0; k < w * 3; ++k ) { uint8_t* b = ( uint8_t* ) &o[k], t0 = b[0], t1 = b[1]; b[0] = b[3]; b[1] = b[2]; b[2] = t1; b[3] = t0; }
    }
    fclose ( f );
    *W = ( size_t ) w; *H = ( size_t ) h;
    return px;
}

/* ---- main ------------------------------------------------------------------------------------ */
static int pick ( const char* v, const char* const* names, int n, int dflt ) { for ( int i = 0; i < n; ++i ) if ( strcmp ( v, names[i] ) == 0 ) return i; return dflt; }

static const char* kHelp =
    "usage: terra_headless scene.obj out.{png,ppm,pfm,hdr} [options]\n"
    "  --width W --height H --spp N --bounces N --integrator simple|direct|mis|normals|depth --tonemap none|linear|reinhard|filmic|uncharted2\n"
    "  --camera px py pz dx dy dz --fov deg --exposure e --gamma g --jitter j --no-flip-z --normals apollo|file\n"
    "  --dump-scene file --no-render --fast-tree | --replica-tree --sample-split n --seed n --tile n\n"
    "  --gpus N (libterra_amd.so only): the scene is replicated on the first N GPUs and the frame's 64-pixel tiles are dealt to them from this one process, one RCCL\n"
    "           gather at the end (terra_amd_set_devices / terra_amd_render_multi); N = 1 runs the same calls on one GPU. Without it: terra_render() on one GPU.\n"
    "  --environment FILE: a lat-long environment map, Radiance .hdr (flat or RLE scanlines, -Y H +X W) or .pfm (either byte order); up to 65535 x 65535\n"
    "  --environment-color R G B: the constant environment when no map is given (default 0.4 0.52 1)\n"
    "  --env-light (libterra_amd.so only): rays that leave the scene add the environment (terra_amd_set_environment_lighting; the reference drops it)\n"
    "  --env-sampling off|table|mis (libterra_amd.so only, with a map and --env-light): table = Direct / Direct + MIS sample the map through a TerraDistribution2D\n"
    "           (terra_amd_set_environment_sampling); mis = that, weighted against Direct + MIS's BSDF ray by the power heuristic (terra_amd_set_environment_mis)\n"
    "  --aov PREFIX (libterra_amd.so only): also runs the first-hit AOV pass with the same calls as the render (terra_amd_render_aov) and writes the means over hits\n"
    "           PREFIX.albedo.pfm, PREFIX.normal.pfm, PREFIX.depth.pfm\n"
    "  --denoise K (libterra_amd.so only): writes the image denoised by K (0 .. 8) a-trous iterations guided by the AOVs (terra_amd_denoise) instead of the plain one\n"
    "  --passes N (libterra_amd.so only): N render calls of --spp samples each, the per-pixel second moments folded after each (terra_amd_accumulate_moments)\n"
    "  --denoise-variance K (libterra_amd.so only): as --denoise, with the colour weight guided by the variance --passes (at least 2) or --adaptive recorded\n"
    "           (terra_amd_denoise_variance)\n"
    "  --adaptive TARGET [--min-passes A --max-passes B] (libterra_amd.so only): passes per --tile (0 = 128) tile until its relative error is at most TARGET\n"
    "           (terra_amd_render_adaptive); the report goes to stderr\n"
    "  --adaptive-masked (with --adaptive, libterra_amd.so only): each round is one masked launch over the active tiles' pixel blocks instead of one call per\n"
    "           tile (terra_amd_render_adaptive_masked); the same rounds and report\n"
    "  --variance out.pfm (libterra_amd.so only): the variance of each pixel's mean luminance after --passes / --adaptive\n"
    "  --frames N [--camera-to px py pz dx dy dz]: N frames, frame f under the camera interpolated linearly between --camera and --camera-to (position and direction;\n"
    "           f / (N - 1) of the way); each frame clears the framebuffer, renders --passes passes and is written to out.0000.ext, out.0001.ext ...\n"
    "           With libterra_amd.so frame f renders under the frame seed --seed + f * 2^32 (terra_amd_set_frame_seed): seeds closer than the frame has pixels\n"
    "           would repeat one noise field, moved along the rows\n"
    "  --temporal ALPHA (libterra_amd.so only, with --frames and --denoise K or --denoise-variance K): each frame also gets its AOV pass and is blended into the\n"
    "           history of the frames before it, reprojected to where each surface lay under the previous camera (terra_amd_reproject; ALPHA in (0, 1], 0 = 0.2);\n"
    "           the blended frame is written through that filter (the variance of --denoise-variance is the history's own)\n"
    "  --camera-model pinhole|thinlens|ortho|equirect|fisheye (libterra_amd.so only; pinhole is the default): the render and AOV calls go through the lens door\n"
    "           (terra_amd_render_lens, terra_amd_render_aov_lens) with --aperture R (thinlens: the lens radius, 0 = pinhole) and --focus D (the distance of the plane\n"
    "           in focus), --ortho-height H (ortho: the world height of the film window), --fisheye-fov DEG (fisheye: the angle across the frame's height, up to 360).\n"
    "           Works with --passes, --aov, --denoise, --denoise-variance, --variance and --frames; not with --adaptive / --gpus (ignored), and --temporal is refused:\n"
    "           reprojection is defined for the pinhole only\n"
    "  --bake-lightmap [--atlas WxH] [--bake-margin M] [--bake-dilate N] (libterra_amd.so only): writes, in place of the camera's image, the irradiance map of the\n"
    "           scene over a W x H texel atlas (default 256x256) as float RGB (.pfm / .hdr): the OBJ's vt times (W, H) are the atlas coordinates, row 0 is v = 0.\n"
    "           terra_amd_atlas_points lays a surface point under every texel whose centre a triangle covers or comes within M texels of (0 .. 4, default 0.5),\n"
    "           terra_amd_render_points gathers --spp cosine-weighted samples per --passes pass at each (PI * sum / samples), terra_amd_dilate grows the lit texels\n"
    "           N passes (0 .. 64, default 2) into the gutters. The camera flags, --aov, --denoise*, --adaptive, --frames and --gpus are ignored.\n"
    "  --bake-probes NXxNYxNZ [--probe-cells N] (libterra_amd.so only): writes, in place of the camera's image, the order-2 spherical harmonics of the radiance\n"
    "           arriving at a grid of NX x NY x NZ light probes, cell-centred over the scene's bounding box (probe (ix, iy, iz) at lo + (i + 0.5) * (hi - lo) / count,\n"
    "           index (iz * NY + iy) * NX + ix), as a float RGB image (.pfm / .hdr) 9 wide and NX * NY * NZ high: pixel (k, p) is coefficient k of probe p.\n"
    "           terra_amd_probe_rays lays N x N (1 .. 64, default 16) equal-area directions about every probe, terra_amd_render_rays gathers --spp samples per\n"
    "           --passes pass along each into one frame, terra_amd_sh_project reduces it. The camera flags, --aov, --denoise*, --adaptive, --frames and --gpus are ignored.\n"
    "  --distance-field NXxNYxNZ PATH (libterra_amd.so only): also writes the scene's distance field as a grey float image (.pfm), NX wide and NY * NZ high: the distance\n"
    "           from the centre of each of NX x NY x NZ cells over the scene's bounding box to the nearest surface (terra_amd_nearest), slice iz in rows iz * NY ..\n"
    "           --signed: the distance is negated in the cells that lie inside the scene's closed surfaces -- three rays to infinity per cell along (0.48, 0.64, 0.60),\n"
    "           (-0.60, 0.48, 0.64) and (0.64, -0.60, 0.48), terra_amd_count_hits on each, inside where at least two of the three counts are odd.\n"
    "  --probe-visibility PATH [--probe-texels M] (with --bake-probes): also writes the probes' visibility maps as a float RGB image (.pfm / .hdr) M * M wide (M 1 .. 16,\n"
    "           default 8) and NX * NY * NZ high: pixel (t, p) is texel t = j * M + i of probe p as (sum of w, sum of w * d, sum of w * d * d), d the distance\n"
    "           terra_amd_intersect finds along the same cell-centre rays, w = cos^64 about the texel's octahedral direction (terra_amd_probe_visibility,\n"
    "           sharpness 6), a miss and the cap being the diagonal of the scene's bounding box.\n"
    "OBJ/MTL import (--normals apollo, the default): the policy of the reference client's importer (satellite/include/Apollo.h under the\n"
    "options of satellite/src/Scene.cpp:83-93) RESTATED in this tool and pinned by hand-derived fixtures -- restated, not executed: Apollo.h\n"
    "does not compile with this image's toolchains. Everything after the TerraObject fill (commit, render, export) is the pinned path.\n";

int main ( int argc, char** argv ) {
    for ( int i = 1; i < argc; ++i ) if ( !strcmp ( argv[i], "--help" ) || !strcmp ( argv[i], "-h" ) ) { fputs ( kHelp, stdout ); return 0; }
    if ( argc < 3 ) { fprintf ( stderr, "usage: terra_headless scene.obj out.{png,ppm,pfm,hdr} [options]\n" ); return 64; }
    if ( terra_amd_init ) ( void ) terra_amd_init();      /* before anything touches the GPU (libterra_amd.so only) */
    size_t W = 800, H = 600, spp = 8, bounces = 4, tile = 0;     /* defaults of satellite/include/Config.hpp:19-113 */
    int integrator = kTerraIntegratorDirect, tonemap = kTerraTonemappingOperatorLinear, flip = 1, fast = -1, have_seed = 0, split = -1, apollo = 1, gpus = 0;
    const char* aov_prefix = NULL; int denoise = -1;
    int passes = 1, denoise_var = -1, min_passes = 0, max_passes = 0, adaptive_masked = 0; float adaptive = 0.f; const char* variance_path = NULL;
    int frames = 0, have_camera_to = 0; float temporal = -1.f; TerraCamera cam_to; memset ( &cam_to, 0, sizeof cam_to );
    const char* dump_path = NULL; int no_render = 0;
    int camera_model = 0; float aperture = 0.f, focus = 1.f, ortho_height = 2.f, fisheye_fov = 180.f;      /* camera_model: 0 pinhole, 1 thinlens, 2 ortho, 3 equirect, 4 fisheye */
    int bake = 0, atlas_w = 256, atlas_h = 256, bake_dilate = 2; float bake_margin = 0.5f;      /* --bake-lightmap */
    int probes_on = 0, probe_n[3] = { 1, 1, 1 }, probe_cells = 16;      /* --bake-probes */
    int field_n[3] = { 0, 0, 0 }; const char* field_path = NULL;        /* --distance-field */
    int field_signed = 0;                                               /* --signed */
    const char* visibility_path = NULL; int probe_texels = 8;      /* --probe-visibility */
    float fov = 45.f, exposure = 1.f, gamma = 2.2f, jitter = 0.f;
    unsigned long long seed = 0;
    const char* env_path = NULL; float env_rgb[3] = { 0.4f, 0.52f, 1.f }; int env_light = 0, env_sampling = 0;      /* env_sampling: 0 off, 1 table, 2 mis */
    TerraCamera cam; cam.position = terra_f3_set ( 0.f, 1.f, -3.4f ); cam.direction = terra_f3_set ( 0.f, 0.f, 1.f ); cam.up = terra_f3_set ( 0.f, 1.f, 0.f );
    for ( int i = 3; i < argc; ++i ) {
        const char* a = argv[i];
#define NEXT() ( i + 1 < argc ? argv[++i] : "" )
        if ( !strcmp ( a, "--width" ) ) W = ( size_t ) atol ( NEXT() );
        else if ( !strcmp ( a, "--height" ) ) H = ( size_t ) atol ( NEXT() );
        else if ( !strcmp ( a, "--spp" ) ) spp = ( size_t ) atol ( NEXT() );
        else if ( !strcmp ( a, "--bounces" ) ) bounces = ( size_t ) atol ( NEXT() );
        else if ( !strcmp ( a, "--tile" ) ) tile = ( size_t ) atol ( NEXT() );
        else if ( !strcmp ( a, "--fov" ) ) fov = ( float ) atof ( NEXT() );
        else if ( !strcmp ( a, "--exposure" ) ) exposure = ( float ) atof ( NEXT() );
        else if ( !strcmp ( a, "--gamma" ) ) gamma = ( float ) atof ( NEXT() );
        else if ( !strcmp ( a, "--jitter" ) ) jitter = ( float ) atof ( NEXT() );
        else if ( !strcmp ( a, "--seed" ) ) { seed = strtoull ( NEXT(), NULL, 0 ); have_seed = 1; }
        else if ( !strcmp ( a, "--no-flip-z" ) ) flip = 0;
        else if ( !strcmp ( a, "--fast-tree" ) ) fast = 1;
        else if ( !strcmp ( a, "--auto-tree" ) ) fast = 2;
        else if ( !strcmp ( a, "--replica-tree" ) ) fast = 0;
        else if ( !strcmp ( a, "--normals" ) ) { const char* v = NEXT(); if ( !strcmp ( v, "apollo" ) ) apollo = 1; else if ( !strcmp ( v, "file" ) ) apollo = 0; else { fprintf ( stderr, "terra_headless: --normals apollo|file\n" ); return 64; } }
        else if ( !strcmp ( a, "--dump-scene" ) ) dump_path = NEXT();
        else if ( !strcmp ( a, "--no-render" ) ) no_render = 1;
        else if ( !strcmp ( a, "--sample-split" ) ) split = atoi ( NEXT() );
        else if ( !strcmp ( a, "--gpus" ) ) gpus = atoi ( NEXT() );
        else if ( !strcmp ( a, "--integrator" ) ) { static const char* const n[] = { "simple", "direct", "mis", "mono", "depth", "normals", "misweights" }; integrator = pick ( NEXT(), n, 7, integrator ); }
        else if ( !strcmp ( a, "--tonemap" ) ) { static const char* const n[] = { "none", "linear", "reinhard", "filmic", "uncharted2" }; tonemap = pick ( NEXT(), n, 5, tonemap ); }
        else if ( !strcmp ( a, "--environment" ) ) env_path = NEXT();
        else if ( !strcmp ( a, "--environment-color" ) && i + 3 < argc ) { for ( int k = 0; k < 3; ++k ) env_rgb[k] = ( float ) atof ( argv[i + 1 + k] ); i += 3; }
        else if ( !strcmp ( a, "--env-light" ) ) env_light = 1;
        else if ( !strcmp ( a, "--aov" ) ) aov_prefix = NEXT();
        else if ( !strcmp ( a, "--denoise" ) ) { denoise = atoi ( NEXT() ); if ( denoise < 0 || denoise > 8 ) { fprintf ( stderr, "terra_headless: --denoise 0 .. 8\n" ); return 64; } }
        else if ( !strcmp ( a, "--passes" ) ) { passes = atoi ( NEXT() ); if ( passes < 1 ) { fprintf ( stderr, "terra_headless: --passes 1 ...\n" ); return 64; } }
        else if ( !strcmp ( a, "--denoise-variance" ) ) { denoise_var = atoi ( NEXT() ); if ( denoise_var < 0 || denoise_var > 8 ) { fprintf ( stderr, "terra_headless: --denoise-variance 0 .. 8\n" ); return 64; } }
        else if ( !strcmp ( a, "--adaptive-masked" ) ) adaptive_masked = 1;
        else if ( !strcmp ( a, "--adaptive" ) ) { adaptive = ( float ) atof ( NEXT() ); if ( !( adaptive > 0.f ) ) { fprintf ( stderr, "terra_headless: --adaptive TARGET > 0\n" ); return 64; } }
        else if ( !strcmp ( a, "--min-passes" ) ) min_passes = atoi ( NEXT() );
        else if ( !strcmp ( a, "--max-passes" ) ) max_passes = atoi ( NEXT() );
        else if ( !strcmp ( a, "--variance" ) ) variance_path = NEXT();
        else if ( !strcmp ( a, "--frames" ) ) { frames = atoi ( NEXT() ); if ( frames < 1 ) { fprintf ( stderr, "terra_headless: --frames 1 ...\n" ); return 64; } }
        else if ( !strcmp ( a, "--temporal" ) ) { temporal = ( float ) atof ( NEXT() ); if ( !( temporal >= 0.f && temporal <= 1.f ) ) { fprintf ( stderr, "terra_headless: --temporal ALPHA in (0, 1], or 0 for 0.2\n" ); return 64; } }
        else if ( !strcmp ( a, "--camera-model" ) ) { static const char* const n[] = { "pinhole", "thinlens", "ortho", "equirect", "fisheye" }; camera_model = pick ( NEXT(), n, 5, -1 ); if ( camera_model < 0 ) { fprintf ( stderr, "terra_headless: --camera-model pinhole|thinlens|ortho|equirect|fisheye\n" ); return 64; } }
        else if ( !strcmp ( a, "--aperture" ) ) aperture = ( float ) atof ( NEXT() );
        else if ( !strcmp ( a, "--focus" ) ) focus = ( float ) atof ( NEXT() );
        else if ( !strcmp ( a, "--ortho-height" ) ) ortho_height = ( float ) atof ( NEXT() );
        else if ( !strcmp ( a, "--fisheye-fov" ) ) fisheye_fov = ( float ) atof ( NEXT() );
        else if ( !strcmp ( a, "--bake-lightmap" ) ) bake = 1;
        else if ( !strcmp ( a, "--atlas" ) ) { if ( sscanf ( NEXT(), "%dx%d", &atlas_w, &atlas_h ) != 2 || atlas_w < 1 || atlas_w > 16384 || atlas_h < 1 || atlas_h > 16384 ) { fprintf ( stderr, "terra_headless: --atlas WxH, each 1 .. 16384\n" ); return 64; } }
        else if ( !strcmp ( a, "--bake-margin" ) ) { bake_margin = ( float ) atof ( NEXT() ); if ( !( bake_margin >= 0.f && bake_margin <= 4.f ) ) { fprintf ( stderr, "terra_headless: --bake-margin 0 .. 4\n" ); return 64; } }
        else if ( !strcmp ( a, "--bake-dilate" ) ) { bake_dilate = atoi ( NEXT() ); if ( bake_dilate < 0 || bake_dilate > 64 ) { fprintf ( stderr, "terra_headless: --bake-dilate 0 .. 64\n" ); return 64; } }
        else if ( !strcmp ( a, "--bake-probes" ) ) {
            probes_on = 1;
            if ( sscanf ( NEXT(), "%dx%dx%d", &probe_n[0], &probe_n[1], &probe_n[2] ) != 3 || probe_n[0] < 1 || probe_n[1] < 1 || probe_n[2] < 1 || ( double ) probe_n[0] * probe_n[1] * probe_n[2] > 1048576. ) { fprintf ( stderr, "terra_headless: --bake-probes NXxNYxNZ, each at least 1, at most 1048576 probes\n" ); return 64; }
        }
        else if ( !strcmp ( a, "--distance-field" ) ) {
            if ( sscanf ( NEXT(), "%dx%dx%d", &field_n[0], &field_n[1], &field_n[2] ) != 3 || field_n[0] < 1 || field_n[1] < 1 || field_n[2] < 1 || ( double ) field_n[0] * field_n[1] * field_n[2] > 16777216. ) { fprintf ( stderr, "terra_headless: --distance-field NXxNYxNZ PATH, each at least 1, at most 16777216 cells\n" ); return 64; }
            field_path = NEXT();
            if ( !*field_path || !strncmp ( field_path, "--", 2 ) ) { fprintf ( stderr, "terra_headless: --distance-field NXxNYxNZ PATH: no path\n" ); return 64; }
        }
        else if ( !strcmp ( a, "--signed" ) ) field_signed = 1;
        else if ( !strcmp ( a, "--probe-visibility" ) ) visibility_path = NEXT();
        else if ( !strcmp ( a, "--probe-texels" ) ) { probe_texels = atoi ( NEXT() ); if ( probe_texels < 1 || probe_texels > 16 ) { fprintf ( stderr, "terra_headless: --probe-texels 1 .. 16\n" ); return 64; } }
        else if ( !strcmp ( a, "--probe-cells" ) ) { probe_cells = atoi ( NEXT() ); if ( probe_cells < 1 || probe_cells > 64 ) { fprintf ( stderr, "terra_headless: --probe-cells 1 .. 64\n" ); return 64; } }
        else if ( !strcmp ( a, "--camera-to" ) && i + 6 < argc ) {
            cam_to.position = terra_f3_set ( ( float ) atof ( argv[i + 1] ), ( float ) atof ( argv[i + 2] ), ( float ) atof ( argv[i + 3] ) );
            cam_to.direction = terra_f3_set ( ( float ) atof ( argv[i + 4] ), ( float ) atof ( argv[i + 5] ), ( float ) atof ( argv[i + 6] ) ); i += 6; have_camera_to = 1;
        }
        else if ( !strcmp ( a, "--env-sampling" ) ) { const char* v = NEXT(); static const char* const n[] = { "off", "table", "mis" }; env_sampling = pick ( v, n, 3, -1 ); if ( env_sampling < 0 ) { fprintf ( stderr, "terra_headless: --env-sampling off|table|mis\n" ); return 64; } }
        else if ( !strcmp ( a, "--camera" ) && i + 6 < argc ) {
            cam.position = terra_f3_set ( ( float ) atof ( argv[i + 1] ), ( float ) atof ( argv[i + 2] ), ( float ) atof ( argv[i + 3] ) );
            cam.direction = terra_f3_set ( ( float ) atof ( argv[i + 4] ), ( float ) atof ( argv[i + 5] ), ( float ) atof ( argv[i + 6] ) ); i += 6;
        } else { fprintf ( stderr, "terra_headless: unknown option %s\n", a ); return 64; }
    }
    cam.fov = fov;
    if ( adaptive_masked && !( adaptive > 0.f ) ) { fprintf ( stderr, "terra_headless: --adaptive-masked is valid only with --adaptive TARGET\n" ); return 64; }
    TerraTexture env_tex; memset ( &env_tex, 0, sizeof env_tex );
    if ( env_path ) {              /* read before the mesh: a bad map is refused before any work */
        size_t ew = 0, eh = 0; char err[128] = "";
        const char* ext = strrchr ( env_path, '.' );
        float* px = ext && ( !strcmp ( ext, ".pfm" ) || !strcmp ( ext, ".PFM" ) ) ? load_pfm ( env_path, &ew, &eh, err, sizeof err ) : load_hdr ( env_path, &ew, &eh, err, sizeof err );
        if ( !px ) { fprintf ( stderr, "terra_headless: %s: %s\n", env_path, err ); return 65; }
        double mean[3] = { 0., 0., 0. };
        for ( size_t k = 0; k < ew * eh; ++k ) for ( int ch = 0; ch < 3; ++ch ) mean[ch] += px[3 * k + ch];
        fprintf ( stderr, "environment: %zu x %zu, mean %.6g %.6g %.6g\n", ew, eh, mean[0] / ( double ) ( ew * eh ), mean[1] / ( double ) ( ew * eh ), mean[2] / ( double ) ( ew * eh ) );
        ( void ) terra_texture_init_hdr ( &env_tex, ew, eh, 3, px );      /* (the reference's returns no value: its result is the pixels it allocated) */
        free ( px );
        if ( !env_tex.pixels ) { fprintf ( stderr, "terra_headless: %s: cannot make a texture of it\n", env_path ); return 65; }
        env_tex.filter = kTerraFilterPoint; env_tex.address_mode = kTerraTextureAddressWrap;
    }
    if ( field_signed && !field_path ) { fprintf ( stderr, "terra_headless: --signed goes with --distance-field NXxNYxNZ PATH\n" ); return 64; }
    if ( field_signed && !terra_amd_count_hits ) { fprintf ( stderr, "terra_headless: --signed needs a libterra_amd.so with terra_amd_count_hits\n" ); return 64; }
    Model m; memset ( &m, 0, sizeof m );
    if ( !load_obj ( &m, argv[1] ) ) { fprintf ( stderr, "terra_headless: no faces in %s\n", argv[1] ); return 66; }
    FILE* dump = dump_path ? fopen ( dump_path, "w" ) : NULL;
    if ( dump_path && !dump ) { fprintf ( stderr, "terra_headless: cannot write %s\n", dump_path ); return 73; }
    HTerraScene scene = apollo ? build_scene_apollo ( &m, flip, dump ) : build_scene ( &m, flip, dump );
    if ( dump ) fclose ( dump );
    if ( no_render ) { printf ( "%s: %zu objects\n", argv[1], terra_scene_count_objects ( scene ) ); terra_scene_destroy ( scene ); return 0; }
    TerraSceneOptions* o = terra_scene_get_options ( scene );
    TerraFloat3 env = terra_f3_set ( env_rgb[0], env_rgb[1], env_rgb[2] );
    if ( env_path ) terra_attribute_init_cubemap ( &o->environment_map, &env_tex );
    else terra_attribute_init_constant ( &o->environment_map, &env );
    o->tonemapping_operator = ( TerraTonemappingOperator ) tonemap; o->accelerator = kTerraAcceleratorBVH; o->sampling_method = kTerraSamplingMethodRandom;
    o->integrator = ( TerraIntegrator ) integrator; o->subpixel_jitter = jitter; o->samples_per_pixel = spp; o->bounces = bounces; o->strata = 4;
    o->manual_exposure = exposure; o->gamma = gamma;
    if ( fast >= 0 && terra_amd_set_tree_mode ) terra_amd_set_tree_mode ( scene, fast );
    if ( split >= 0 && terra_amd_set_sample_split ) terra_amd_set_sample_split ( scene, split );
    if ( have_seed && terra_amd_set_frame_seed ) terra_amd_set_frame_seed ( scene, seed );
    if ( env_light || env_sampling ) {
        if ( !terra_amd_set_environment_lighting || !terra_amd_set_environment_sampling || !terra_amd_set_environment_mis )
            fprintf ( stderr, "terra_headless: --env-light / --env-sampling need libterra_amd.so (this library drops the environment term); ignored\n" );
        else {
            if ( env_light ) terra_amd_set_environment_lighting ( scene, 1 );
            terra_amd_set_environment_sampling ( scene, env_sampling != 0 );
            terra_amd_set_environment_mis ( scene, env_sampling == 2 );
        }
    }
    if ( gpus > 0 ) {          /* several GPUs from this one process: the first `gpus` devices, the first of them primary */
        int devs[64];
        if ( !terra_amd_set_devices || !terra_amd_render_multi ) { fprintf ( stderr, "terra_headless: --gpus needs libterra_amd.so\n" ); return 64; }
        if ( gpus > 64 || ( terra_amd_device_count && gpus > terra_amd_device_count() ) ) { fprintf ( stderr, "terra_headless: --gpus %d but %d visible\n", gpus, terra_amd_device_count ? terra_amd_device_count() : 0 ); return 69; }
        for ( int k = 0; k < gpus; ++k ) devs[k] = k;
        if ( terra_amd_set_devices ( devs, gpus ) != 0 ) { fprintf ( stderr, "terra_headless: %s\n", terra_amd_last_error ? terra_amd_last_error() : "terra_amd_set_devices failed" ); return 69; }
    }
    if ( field_path && ( !terra_amd_scene_vertex_points || !terra_amd_nearest ) ) { fprintf ( stderr, "terra_headless: --distance-field needs libterra_amd.so; ignored\n" ); field_path = NULL; }
    if ( field_path ) {          /* beside whatever else the run writes: the distance to the nearest surface at the centres of NX x NY x NZ cells over the bounding box */
        const size_t nx = ( size_t ) field_n[0], ny = ( size_t ) field_n[1], nz = ( size_t ) field_n[2], n = nx * ny * nz;
        terra_scene_commit ( scene );
        const int nv = terra_amd_scene_vertex_points ( scene, NULL, 0 );
        if ( nv <= 0 ) { fprintf ( stderr, "terra_headless: --distance-field: the scene has no triangles\n" ); return 66; }
        BakePoint* verts = aligned_alloc ( 16, ( size_t ) nv * sizeof ( BakePoint ) );
        NearestQuery* queries = aligned_alloc ( 16, n * sizeof ( NearestQuery ) ); NearestAnswer* answers = aligned_alloc ( 16, n * sizeof ( NearestAnswer ) );
        TerraFramebuffer field;
        if ( !verts || !queries || !answers || !terra_framebuffer_create ( &field, nx, ny * nz ) ) { fprintf ( stderr, "terra_headless: out of memory\n" ); return 71; }
        int rc = terra_amd_scene_vertex_points ( scene, verts, nv ) < 0;
        float lo[3], sp[3];
        ( void ) cell_grid_over ( verts, nv, field_n, lo, sp );
        for ( size_t iz = 0; iz < nz; ++iz ) for ( size_t iy = 0; iy < ny; ++iy ) for ( size_t ix = 0; ix < nx; ++ix ) {
            NearestQuery* q = &queries[ ( iz * ny + iy ) * nx + ix];
            const size_t i[3] = { ix, iy, iz };
            for ( int a = 0; a < 3; ++a ) { volatile float t = ( ( float ) i[a] + 0.5f ) * sp[a]; q->position[a] = t + lo[a]; }          /* (volatile: multiply, then add -- no fused form) */
            q->max_distance = INFINITY;
        }
        if ( !rc ) rc = terra_amd_nearest ( scene, queries, n, answers );
        if ( rc ) { fprintf ( stderr, "terra_headless: %s\n", terra_amd_last_error && *terra_amd_last_error() ? terra_amd_last_error() : "the distance field failed" ); return 70; }
        if ( field_signed ) {          /* the crossing sign: three rays to infinity per cell, inside where at least two of the three counts are odd */
            static const float dirs[3][3] = { { 0.48f, 0.64f, 0.60f }, { -0.60f, 0.48f, 0.64f }, { 0.64f, -0.60f, 0.48f } };
            QueryRay* rays = aligned_alloc ( 16, 3 * n * sizeof ( QueryRay ) ); uint32_t* counts = malloc ( 3 * n * sizeof ( uint32_t ) );
            if ( !rays || !counts ) { fprintf ( stderr, "terra_headless: out of memory\n" ); return 71; }
            for ( int v = 0; v < 3; ++v ) for ( size_t k = 0; k < n; ++k ) {
                QueryRay* r = &rays[ ( size_t ) v * n + k];
                for ( int a = 0; a < 3; ++a ) { r->origin[a] = queries[k].position[a]; r->direction[a] = dirs[v][a]; }
                r->tmax = INFINITY; r->reserved = 0.f;
            }
            if ( terra_amd_count_hits ( scene, rays, 3 * n, counts ) ) { fprintf ( stderr, "terra_headless: %s\n", terra_amd_last_error && *terra_amd_last_error() ? terra_amd_last_error() : "the crossing counts failed" ); return 70; }
            size_t inside = 0;
            for ( size_t k = 0; k < n; ++k ) if ( ( counts[k] & 1u ) + ( counts[n + k] & 1u ) + ( counts[2 * n + k] & 1u ) >= 2u ) { answers[k].distance = -answers[k].distance; ++inside; }
            printf ( "%s: signed by crossings: %zu of %zu cells inside\n", argv[1], inside, n );
            free ( rays ); free ( counts );
        }
        for ( size_t k = 0; k < n; ++k ) field.pixels[k] = terra_f3_set ( answers[k].distance, answers[k].distance, answers[k].distance );          /* slice iz = rows iz * NY .. of the image */
        if ( !write_pfm ( field_path, &field ) ) { fprintf ( stderr, "terra_headless: cannot write %s\n", field_path ); return 73; }
        printf ( "%s: distance field %s (%dx%dx%d cells from %g %g %g, spacing %g %g %g)\n", argv[1], field_path, field_n[0], field_n[1], field_n[2], ( double ) lo[0], ( double ) lo[1], ( double ) lo[2], ( double ) sp[0], ( double ) sp[1], ( double ) sp[2] );
        free ( verts ); free ( queries ); free ( answers ); terra_framebuffer_destroy ( &field );
    }
    if ( bake && ( !terra_amd_atlas_points || !terra_amd_render_points || !terra_amd_dilate ) ) { fprintf ( stderr, "terra_headless: --bake-lightmap needs libterra_amd.so; ignored, the camera's image is written\n" ); bake = 0; }
    if ( bake ) {          /* the atlas is the frame: points under the texels, irradiance at the points, the lit texels grown into the gutters */
        const size_t aw = ( size_t ) atlas_w, ah = ( size_t ) atlas_h, n = aw * ah;
        terra_scene_commit ( scene );
        BakeAtlas atlas; memset ( &atlas, 0, sizeof atlas );
        atlas.width = atlas_w; atlas.height = atlas_h; atlas.uv_scale[0] = ( float ) atlas_w; atlas.uv_scale[1] = ( float ) atlas_h; atlas.margin = bake_margin;
        BakeSampling cosine; memset ( &cosine, 0, sizeof cosine );
        BakePoint* points = aligned_alloc ( 16, n * sizeof ( BakePoint ) ); BakeTexel* texels = malloc ( n * sizeof ( BakeTexel ) ); int* valid = malloc ( n * sizeof ( int ) );
        TerraFramebuffer lm;
        if ( !points || !texels || !valid || !terra_framebuffer_create ( &lm, aw, ah ) ) { fprintf ( stderr, "terra_headless: out of memory\n" ); return 71; }
        int rc = terra_amd_atlas_points ( scene, &atlas, NULL, points, texels );
        for ( int pass = 0; pass < passes && !rc; ++pass ) rc = terra_amd_render_points ( scene, &cosine, points, &lm, 0, 0, aw, ah );
        size_t covered = 0;
        for ( size_t i = 0; i < n && !rc; ++i ) {
            const TerraRawIntegrationResult* r = &lm.results[i];
            const float s = ( float ) r->samples;
            lm.pixels[i] = terra_f3_set ( 3.14159274f * r->acc.x / s, 3.14159274f * r->acc.y / s, 3.14159274f * r->acc.z / s );
            valid[i] = texels[i].triangle >= 0; covered += ( size_t ) valid[i];
        }
        if ( !rc ) rc = terra_amd_dilate ( &lm.pixels[0].x, 3, valid, atlas_w, atlas_h, bake_dilate );
        if ( rc ) { fprintf ( stderr, "terra_headless: %s\n", terra_amd_last_error && *terra_amd_last_error() ? terra_amd_last_error() : "the bake failed" ); return 70; }
        if ( !write_image ( argv[2], &lm ) ) { fprintf ( stderr, "terra_headless: cannot write %s\n", argv[2] ); return 73; }
        printf ( "%s: %zu triangles, %zu materials -> lightmap %s (%zux%zu texels, %zu covered, %zu spp x %d)\n", argv[1], m.faces.n, m.mtls.n, argv[2], aw, ah, covered, spp, passes );
        free ( points ); free ( texels ); free ( valid );
        terra_framebuffer_destroy ( &lm );
        terra_scene_destroy ( scene );
        if ( env_path ) terra_texture_destroy ( &env_tex );
        return 0;
    }
    if ( probes_on && ( !terra_amd_scene_vertex_points || !terra_amd_probe_grid_points || !terra_amd_probe_rays || !terra_amd_render_rays || !terra_amd_sh_project ) ) {
        fprintf ( stderr, "terra_headless: --bake-probes needs libterra_amd.so; ignored, the camera's image is written\n" ); probes_on = 0;
    }
    if ( visibility_path && !probes_on ) { fprintf ( stderr, "terra_headless: --probe-visibility goes with --bake-probes; ignored\n" ); visibility_path = NULL; }
    if ( visibility_path && ( !terra_amd_intersect || !terra_amd_probe_visibility ) ) { fprintf ( stderr, "terra_headless: --probe-visibility needs libterra_amd.so; ignored\n" ); visibility_path = NULL; }
    if ( probes_on ) {          /* the probe frame: cell c of probe p at pixel (c, p); one projection of everything the passes gathered */
        const size_t P = ( size_t ) probe_n[0] * ( size_t ) probe_n[1] * ( size_t ) probe_n[2], K = ( size_t ) probe_cells * ( size_t ) probe_cells;
        terra_scene_commit ( scene );
        const int nv = terra_amd_scene_vertex_points ( scene, NULL, 0 );
        BakePoint* verts = nv > 0 ? aligned_alloc ( 16, ( size_t ) nv * sizeof ( BakePoint ) ) : NULL;
        BakePoint* probes = aligned_alloc ( 16, P * sizeof ( BakePoint ) ); ProbeRay* rays = aligned_alloc ( 16, P * K * sizeof ( ProbeRay ) ); ProbeSH* sh = aligned_alloc ( 16, P * sizeof ( ProbeSH ) );
        TerraFramebuffer frame, image;
        if ( !verts || !probes || !rays || !sh || !terra_framebuffer_create ( &frame, K, P ) || !terra_framebuffer_create ( &image, 9, P ) ) { fprintf ( stderr, "terra_headless: out of memory\n" ); return 71; }
        int rc = terra_amd_scene_vertex_points ( scene, verts, nv ) < 0;
        ProbeGrid grid; memset ( &grid, 0, sizeof grid );
        grid.nx = probe_n[0]; grid.ny = probe_n[1]; grid.nz = probe_n[2];
        float lo[3], sp[3];
        const double diagonal2 = cell_grid_over ( verts, nv, probe_n, lo, sp );          /* of the bounding box, for --probe-visibility */
        for ( int a = 0; a < 3; ++a ) { grid.spacing[a] = sp[a]; grid.origin[a] = lo[a] + 0.5f * sp[a]; }          /* cell-centred over the bounding box */
        if ( !rc ) rc = terra_amd_probe_grid_points ( &grid, probes, ( int ) P ) < 0;
        if ( !rc ) rc = terra_amd_probe_rays ( probes, P, probe_cells, NULL, rays );
        for ( int pass = 0; pass < passes && !rc; ++pass ) rc = terra_amd_render_rays ( scene, rays, &frame, 0, 0, K, P );
        if ( !rc ) rc = terra_amd_sh_project ( &frame, rays, P, probe_cells, 0, sh );
        if ( rc ) { fprintf ( stderr, "terra_headless: %s\n", terra_amd_last_error && *terra_amd_last_error() ? terra_amd_last_error() : "the probe bake failed" ); return 70; }
        for ( size_t p = 0; p < P; ++p ) for ( int k = 0; k < 9; ++k ) image.pixels[9 * p + ( size_t ) k] = terra_f3_set ( sh[p].c[k][0], sh[p].c[k][1], sh[p].c[k][2] );
        if ( !write_image ( argv[2], &image ) ) { fprintf ( stderr, "terra_headless: cannot write %s\n", argv[2] ); return 73; }
        if ( visibility_path ) {          /* the distances along the same cell-centre rays, filtered into one map per probe */
            const size_t MM = ( size_t ) probe_texels * ( size_t ) probe_texels;
            ProbeHit* hits = aligned_alloc ( 16, P * K * sizeof ( ProbeHit ) ); VisibilityTexel* texels = aligned_alloc ( 16, P * MM * sizeof ( VisibilityTexel ) );
            TerraFramebuffer maps;
            if ( !hits || !texels || !terra_framebuffer_create ( &maps, MM, P ) ) { fprintf ( stderr, "terra_headless: out of memory\n" ); return 71; }
            ProbeVisibility vis; memset ( &vis, 0, sizeof vis );
            vis.texels = probe_texels; vis.sharpness = 6; vis.max_distance = ( float ) sqrt ( diagonal2 );
            rc = terra_amd_intersect ( scene, rays, P * K, hits );
            if ( !rc ) rc = terra_amd_probe_visibility ( hits, rays, P, probe_cells, &vis, 0, texels );
            if ( rc ) { fprintf ( stderr, "terra_headless: %s\n", terra_amd_last_error && *terra_amd_last_error() ? terra_amd_last_error() : "the probe visibility bake failed" ); return 70; }
            for ( size_t t = 0; t < P * MM; ++t ) maps.pixels[t] = terra_f3_set ( texels[t].weight, texels[t].distance, texels[t].distance2 );
            if ( !write_image ( visibility_path, &maps ) ) { fprintf ( stderr, "terra_headless: cannot write %s\n", visibility_path ); return 73; }
            printf ( "%s: probe visibility %s (%d x %d texels, max distance %g)\n", argv[1], visibility_path, probe_texels, probe_texels, ( double ) vis.max_distance );
            free ( hits ); free ( texels ); terra_framebuffer_destroy ( &maps );
        }
        printf ( "%s: %zu triangles, %zu materials -> probes %s (%dx%dx%d probes, %d x %d cells, %zu spp x %d)\n", argv[1], m.faces.n, m.mtls.n, argv[2], probe_n[0], probe_n[1], probe_n[2], probe_cells, probe_cells, spp, passes );
        free ( verts ); free ( probes ); free ( rays ); free ( sh );
        terra_framebuffer_destroy ( &frame ); terra_framebuffer_destroy ( &image );
        terra_scene_destroy ( scene );
        if ( env_path ) terra_texture_destroy ( &env_tex );
        return 0;
    }
    Lens lens; memset ( &lens, 0, sizeof lens );          /* --camera-model: the lens door's camera model */
    if ( camera_model > 0 ) {
        if ( temporal >= 0.f ) { fprintf ( stderr, "terra_headless: --temporal with --camera-model other than pinhole: reprojection is defined for the pinhole camera only\n" ); return 64; }
        if ( !terra_amd_render_lens || !terra_amd_render_aov_lens ) fprintf ( stderr, "terra_headless: --camera-model needs libterra_amd.so; ignored, the pinhole image is written\n" );
        else {
            lens.model = camera_model - 1;
            if ( camera_model == 1 ) { lens.lens_radius = aperture; lens.focus_distance = focus; }
            if ( camera_model == 2 ) lens.ortho_height = ortho_height;
            if ( camera_model == 4 ) lens.fisheye_fov = fisheye_fov;
            g_lens = &lens;
            if ( gpus > 0 || adaptive > 0.f ) { fprintf ( stderr, "terra_headless: --camera-model does not mirror --gpus / --adaptive; those are ignored\n" ); gpus = 0; adaptive = 0.f; }
        }
    }
    if ( adaptive_masked && !terra_amd_render_adaptive_masked ) { fprintf ( stderr, "terra_headless: --adaptive-masked needs libterra_amd.so; ignored\n" ); adaptive_masked = 0; }
    MomentSum* mom = NULL;       /* --passes / --denoise-variance / --adaptive / --variance: the second moments of the batch means */
    if ( passes > 1 || denoise_var >= 0 || adaptive > 0.f || variance_path ) {
        const char* why = ( !terra_amd_accumulate_moments || !terra_amd_denoise_variance || !terra_amd_render_adaptive || !terra_amd_render_aov ) ? "need libterra_amd.so" : gpus > 0 ? "do not mirror --gpus (the sharded render)" : NULL;
        if ( why ) { fprintf ( stderr, "terra_headless: --passes / --denoise-variance / --adaptive / --variance %s; ignored, the plain image is written\n", why ); passes = 1; denoise_var = -1; adaptive = 0.f; variance_path = NULL; }
        else if ( !( mom = calloc ( W * H, sizeof ( MomentSum ) ) ) ) { fprintf ( stderr, "terra_headless: out of memory\n" ); return 71; }
    }
    AovSum* aov = NULL;          /* --aov / --denoise: the AOV sums, made by the same calls as the render */
    if ( aov_prefix || denoise >= 0 || denoise_var >= 0 ) {
        if ( !terra_amd_render_aov || !terra_amd_denoise ) { fprintf ( stderr, "terra_headless: --aov / --denoise need libterra_amd.so; ignored, the plain image is written\n" ); aov_prefix = NULL; denoise = -1; }
        else if ( gpus > 0 ) { fprintf ( stderr, "terra_headless: --aov / --denoise do not mirror --gpus (the sharded render); ignored\n" ); aov_prefix = NULL; denoise = -1; }
        else if ( !( aov = calloc ( W * H, sizeof ( AovSum ) ) ) ) { fprintf ( stderr, "terra_headless: out of memory\n" ); return 71; }
    }
    if ( ( have_camera_to || temporal >= 0.f ) && frames < 1 ) { fprintf ( stderr, "terra_headless: --camera-to / --temporal go with --frames N; ignored\n" ); temporal = -1.f; }
    if ( frames >= 1 && ( gpus > 0 || adaptive > 0.f ) ) { fprintf ( stderr, "terra_headless: --frames does not mirror --gpus / --adaptive; ignored, one frame is written\n" ); frames = 0; temporal = -1.f; }
    if ( frames >= 1 ) {          /* every flag the frames path does not act on is reported, as the other extension flags are */
        if ( temporal >= 0.f && !terra_amd_reproject ) { fprintf ( stderr, "terra_headless: --temporal needs libterra_amd.so; ignored, the plain frames are written\n" ); temporal = -1.f; }
        if ( temporal >= 0.f && denoise < 0 && denoise_var < 0 ) {
            fprintf ( stderr, "terra_headless: --temporal writes the blended frame through --denoise K or --denoise-variance K and neither is given; ignored, the plain frames are written\n" );
            temporal = -1.f;
        }
        if ( temporal < 0.f && ( denoise >= 0 || denoise_var >= 0 ) ) { fprintf ( stderr, "terra_headless: --denoise / --denoise-variance with --frames go with --temporal; ignored, the plain frames are written\n" ); denoise = -1; denoise_var = -1; }
        if ( aov_prefix || variance_path ) { fprintf ( stderr, "terra_headless: --aov / --variance are not written with --frames; ignored\n" ); aov_prefix = NULL; variance_path = NULL; }
    }
    terra_scene_commit ( scene );
    TerraFramebuffer fb;
    if ( !terra_framebuffer_create ( &fb, W, H ) ) { fprintf ( stderr, "terra_headless: bad framebuffer size\n" ); return 65; }
    if ( frames >= 1 ) {            /* a camera move: one image per frame, each blended into the reprojected history of those before it */
        const int blend = temporal >= 0.f;
        HistoryEntry* hist[2] = { NULL, NULL }; TerraRawIntegrationResult* chained = NULL; MomentSum* hmom = NULL;
        if ( blend ) {
            if ( !aov ) aov = calloc ( W * H, sizeof ( AovSum ) );
            hist[0] = calloc ( W * H, sizeof ( HistoryEntry ) ); hist[1] = calloc ( W * H, sizeof ( HistoryEntry ) );
            chained = calloc ( W * H, sizeof ( TerraRawIntegrationResult ) ); hmom = calloc ( W * H, sizeof ( MomentSum ) );
            if ( !aov || !hist[0] || !hist[1] || !chained || !hmom ) { fprintf ( stderr, "terra_headless: out of memory\n" ); return 71; }
        }
        if ( !have_camera_to ) { cam_to.position = cam.position; cam_to.direction = cam.direction; }
        const char* ext = strrchr ( argv[2], '.' ); if ( !ext || strchr ( ext, '/' ) ) ext = argv[2] + strlen ( argv[2] );
        TerraCamera prev = cam;
        /* Each frame draws its own random numbers. The device keys a pixel's stream with (frame seed + pixel index, samples so far), and the clear below sets the
           last back to 0: under one seed every frame would repeat the first one's noise and the history would average copies, and under seed + f frame f would be
           frame 0's noise moved by f pixels (seed + f at pixel p is seed at pixel p + f). Two seeds give independent frames only if they lie further apart than
           the frame has pixels, so frame f renders under seed + f * 2^32 (frame 0 under --seed or the library's default: --frames 1 is the plain run). The
           reference seeds itself from the clock. */
        const uint64_t seed0 = have_seed ? ( uint64_t ) seed : terra_amd_get_frame_seed ? terra_amd_get_frame_seed ( scene ) : 0;
        for ( int f = 0; f < frames; ++f ) {
            if ( terra_amd_set_frame_seed ) terra_amd_set_frame_seed ( scene, seed0 + ( ( uint64_t ) f << 32 ) );
            const float t = frames > 1 ? ( float ) f / ( float ) ( frames - 1 ) : 0.f;
            TerraCamera cf = cam;
            cf.position = terra_f3_set ( cam.position.x + ( cam_to.position.x - cam.position.x ) * t, cam.position.y + ( cam_to.position.y - cam.position.y ) * t, cam.position.z + ( cam_to.position.z - cam.position.z ) * t );
            cf.direction = terra_f3_set ( cam.direction.x + ( cam_to.direction.x - cam.direction.x ) * t, cam.direction.y + ( cam_to.direction.y - cam.direction.y ) * t, cam.direction.z + ( cam_to.direction.z - cam.direction.z ) * t );
            terra_framebuffer_clear ( &fb );
            if ( aov ) memset ( aov, 0, W * H * sizeof ( AovSum ) );
            for ( int pass = 0; pass < passes; ++pass ) {
                const size_t tl = tile ? tile : ( W > H ? W : H );
                for ( size_t y = 0; y < H; y += tl ) for ( size_t x = 0; x < W; x += tl ) {
                    const size_t tw = W - x < tl ? W - x : tl, th = H - y < tl ? H - y : tl;
                    render_rect ( &cf, scene, &fb, x, y, tw, th );
                    if ( aov ) render_aov_rect ( &cf, scene, aov, W, H, x, y, tw, th );
                }
            }
            if ( terra_amd_last_error && *terra_amd_last_error() ) { fprintf ( stderr, "terra_headless: %s\n", terra_amd_last_error() ); return 70; }
            if ( blend ) {
                TemporalOptions to = { temporal, 0.f, 0.f, 0 };
                TerraFramebuffer cfb = fb; cfb.results = chained;
                int rc = terra_amd_reproject ( scene, &cf, &prev, &fb, aov, f ? hist[( f + 1 ) & 1] : NULL, hist[f & 1], chained, hmom, 0, 0, W, H, &to );
                if ( !rc ) rc = denoise_var >= 0 ? terra_amd_denoise_variance ( scene, &cfb, aov, hmom, 0, 0, W, H, denoise_var, NULL, fb.pixels )
                                                 : terra_amd_denoise ( scene, &cfb, aov, 0, 0, W, H, denoise, NULL, fb.pixels );
                if ( rc ) { fprintf ( stderr, "terra_headless: %s\n", terra_amd_last_error ? terra_amd_last_error() : "reproject failed" ); return 70; }
            }
            char path[4096];
            snprintf ( path, sizeof path, "%.*s.%04d%s", ( int ) ( ext - argv[2] ), argv[2], f, ext );
            if ( !write_image ( path, &fb ) ) { fprintf ( stderr, "terra_headless: cannot write %s\n", path ); return 73; }
            prev = cf;
        }
        printf ( "%s: %zu triangles, %zu materials -> %d frames %.*s.0000%s ... (%zux%zu, %zu spp)\n", argv[1], m.faces.n, m.mtls.n, frames, ( int ) ( ext - argv[2] ), argv[2], ext, W, H, spp );
        free ( aov ); free ( mom ); free ( hist[0] ); free ( hist[1] ); free ( chained ); free ( hmom );
        terra_framebuffer_destroy ( &fb );
        terra_scene_destroy ( scene );
        if ( env_path ) terra_texture_destroy ( &env_tex );
        return 0;
    }
    if ( mom && adaptive > 0.f ) {
        AdaptiveOptions ao = { tile, min_passes, max_passes, adaptive, 0 }; AdaptiveReport ar; memset ( &ar, 0, sizeof ar );
        if ( ( adaptive_masked ? terra_amd_render_adaptive_masked : terra_amd_render_adaptive ) ( &cam, scene, &fb, mom, aov, 0, 0, W, H, &ao, &ar ) != 0 ) { fprintf ( stderr, "terra_headless: %s\n", terra_amd_last_error && *terra_amd_last_error() ? terra_amd_last_error() : "terra_amd_render_adaptive failed" ); return 70; }
        fprintf ( stderr, "adaptive%s: %d rounds, %llu tile calls, %llu samples, %d of %d tiles at or below %g, largest error left %g%s\n", adaptive_masked ? " (masked launches)" : "", ar.rounds, ( unsigned long long ) ar.tile_calls,
                      ( unsigned long long ) ar.samples, ar.tiles_converged, ar.tiles, ( double ) adaptive, ( double ) ar.max_error, ar.hit_max_batches ? " (--max-passes ended it)" : "" );
    } else if ( mom ) for ( int pass = 0; pass < passes; ++pass ) {
        const size_t t = tile ? tile : ( W > H ? W : H );
        for ( size_t y = 0; y < H; y += t ) for ( size_t x = 0; x < W; x += t ) {
            const size_t tw = W - x < t ? W - x : t, th = H - y < t ? H - y : t;
            render_rect ( &cam, scene, &fb, x, y, tw, th );
            if ( aov ) render_aov_rect ( &cam, scene, aov, W, H, x, y, tw, th );
        }
        ( void ) terra_amd_accumulate_moments ( scene, &fb, mom, 0, 0, W, H );
    }
    else if ( gpus > 0 ) ( void ) terra_amd_render_multi ( &cam, scene, &fb, 0, 0, W, H, tile );      /* (tile = the shard's tile size here; 0 = 64) */
    else if ( tile == 0 ) { render_rect ( &cam, scene, &fb, 0, 0, W, H ); if ( aov ) render_aov_rect ( &cam, scene, aov, W, H, 0, 0, W, H ); }
    else for ( size_t y = 0; y < H; y += tile ) for ( size_t x = 0; x < W; x += tile ) {
        const size_t tw = W - x < tile ? W - x : tile, th = H - y < tile ? H - y : tile;
        render_rect ( &cam, scene, &fb, x, y, tw, th );
        if ( aov ) render_aov_rect ( &cam, scene, aov, W, H, x, y, tw, th );
    }
    if ( terra_amd_last_error && *terra_amd_last_error() ) { fprintf ( stderr, "terra_headless: %s\n", terra_amd_last_error() ); return 70; }
    if ( aov_prefix ) {
        static const char* const kind[3] = { "albedo", "normal", "depth" };
        for ( int k = 0; k < 3; ++k ) {
            char path[4096];
            snprintf ( path, sizeof path, "%s.%s.pfm", aov_prefix, kind[k] );
            if ( !write_aov_pfm ( path, aov, W, H, k ) ) { fprintf ( stderr, "terra_headless: cannot write %s\n", path ); return 73; }
        }
    }
    if ( denoise >= 0 && terra_amd_denoise ( scene, &fb, aov, 0, 0, W, H, denoise, NULL, fb.pixels ) != 0 ) { fprintf ( stderr, "terra_headless: %s\n", terra_amd_last_error ? terra_amd_last_error() : "denoise failed" ); return 70; }
    if ( variance_path && !write_variance_pfm ( variance_path, mom, W, H ) ) { fprintf ( stderr, "terra_headless: cannot write %s\n", variance_path ); return 73; }
    if ( denoise_var >= 0 && terra_amd_denoise_variance ( scene, &fb, aov, mom, 0, 0, W, H, denoise_var, NULL, fb.pixels ) != 0 ) { fprintf ( stderr, "terra_headless: %s\n", terra_amd_last_error ? terra_amd_last_error() : "denoise failed" ); return 70; }
    free ( aov ); free ( mom );
    if ( !write_image ( argv[2], &fb ) ) { fprintf ( stderr, "terra_headless: cannot write %s\n", argv[2] ); return 73; }
    printf ( "%s: %zu triangles, %zu materials -> %s (%zux%zu, %zu spp)\n", argv[1], m.faces.n, m.mtls.n, argv[2], W, H, spp );
    terra_framebuffer_destroy ( &fb );
    terra_scene_destroy ( scene );
    if ( env_path ) terra_texture_destroy ( &env_tex );
    return 0;
}
