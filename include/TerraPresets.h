/*
 * TerraPresets.h -- built-in BSDF presets (drop-in boundary, part 3 of 3).
 *
 * Same names and attribute-slot numbers as reference include/TerraPresets.h:11-33.
 * terra_bsdf_*_init() stores the library's own sample/pdf/eval entry points in
 * the TerraBSDF; terra_scene_commit() recognises those pointers and selects the
 * matching device BSDF ("Function-pointer plug-ins").
 *
 * The sample/pdf/eval entry points themselves are exported (as in the
 * reference, src/TerraPresets.c:34,47,52,84,108,125) as *markers*: calling
 * them on the host is not supported -- they log an error and return zero --
 * because this library has no CPU shading path.
 */
#ifndef TERRA_AMD_TERRA_PRESETS_H
#define TERRA_AMD_TERRA_PRESETS_H

#include "Terra.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Lambertian, cosine-weighted sampling. attributes[0] = albedo. */
#define TERRA_DIFFUSE_ALBEDO 0
#define TERRA_DIFFUSE_END    1
void terra_bsdf_diffuse_init ( TerraBSDF* bsdf );

typedef struct {
    TerraFloat3 albedo;
} TerraMaterialDiffuse;

/* Modified Phong. Slot 3 is scratch written by sample() and read by pdf(). */
#define TERRA_PHONG_SPECULAR_COLOR     0
#define TERRA_PHONG_ALBEDO             1
#define TERRA_PHONG_SPECULAR_INTENSITY 2
#define TERRA_PHONG_SAMPLE_PICK        3
#define TERRA_PHONG_END                4
void terra_bsdf_phong_init ( TerraBSDF* bsdf );

typedef struct {
    TerraFloat3 albedo;
    TerraFloat3 specular_color;
    float       specular_intensity;
    bool        sample_diffuse;
} TerraMaterialPhong;

/* ---- presets the reference does not have in runnable form ------------------------------
 * BASELINE.json config 4 asks for a GGX metal and a dielectric glass. The reference only
 * contains dead code for them (src/TerraPresets.c:298-465, inside #if 0, written against a
 * removed API), so there is NO reference behaviour to match: these two presets are DEFINED
 * here, in the live sample/pdf/eval form, from that code's building blocks (GGX D :316-320,
 * Smith G1 :307-314, half-vector sampling :333-343, Snell/TIR/Schlick :399-449). Parity for
 * They have no reference behaviour; they are pinned to a binary64 statement of the rules below
 * (tests/presets_ref.py), and the device to this repo's oracle bit for bit.
 *
 * GGX conductor:  attributes[0] = F0 (specular colour), attributes[1].x = roughness alpha.
 * Glass:          attributes[0] = tint, material.ior = index of refraction; attributes[2]
 *                 and attributes[3].x are scratch written by sample() (the chosen direction and
 *                 its probability), like Phong's slot 3.
 *
 * THE RULES. n is the shading normal, wo points away from the surface towards where the path came
 * from, wi is the direction the path continues in; all unit vectors. Everything is binary32.
 * "pi" is terra_PI (TerraMath.h), the reference's 3.1416926535f, 1e-4 above pi: the azimuth goes through
 * the path the diffuse sampler uses (one variate -> sin/cos of 2 terra_PI e), and D is normalised by
 * the same constant. The stated pdf therefore integrates to 1 - 3.2e-5 over its lobe.
 *
 * GGX, alpha in [0.001, 1]:
 *   sample (e1, e2):  t2 = alpha^2 e1 / (1 - e1)  (tan^2 of the half vector's polar angle),
 *       cos_t = 1 / sqrt (1 + t2),  sin_t = sqrt (t2) cos_t  (NOT sqrt (1 - cos_t^2): that cancels),
 *       phi = 2 pi e2,  local h = (sin_t cos phi, cos_t, sin_t sin phi),  h = normalize (M h) with M the
 *       surface's transform, whose columns are (tangent, n, bitangent) as terra_f4x4_basis makes them.
 *       That basis is the reference's: tangent and bitangent have length k^2 = 1 - (the smaller of
 *       nx^2, ny^2), in [1/2, 1], not 1, so about a normal that is not axis-aligned the lobe the
 *       sampler draws is narrower by up to k^2 in tan (theta_h) than the one pdf() states. Intended:
 *       the diffuse and Phong presets sample through the same basis by reference parity, and an
 *       axis-aligned normal (every wall of a Cornell box) has k = 1.
 *       wi = 2 max (0, h.wo) h - wo. A half vector that faces away from wo therefore gives wi = -wo
 *       exactly ("clamped"); pdf and eval are 0 there and the path dies. e1 = 0 gives h = n and wi
 *       the mirror direction.
 *   pdf (wi, wo):  h = normalize (wi + wo);  0 unless h.wo > 0 -- NaN included, so wi = -wo gives 0 --
 *       else D (n.h) (n.h) / (4 h.wo),  D (c) = alpha^2 / (pi (c^2 alpha^2 + 1 - c^2)^2) for c > 0, else 0.
 *   eval (wi, wo): 0 unless n.wi > 0 and n.wo > 0; else F G D / (4 n.wi n.wo) with
 *       F = F0 + (1 - F0) max (0, 1 - max (0, h.wo))^5 per channel (h.wo can round above 1),  G = G1 (wo) G1 (wi),
 *       G1 (v) = 2 / (1 + sqrt (1 + alpha^2 tan^2 (v, n))) where (v.h) / (v.n) > 0, else 0.
 *       In binary32 the relative error of D grows as 2^-23 / (c^2 alpha^2 + 1 - c^2) -- the sum cancels --
 *       i.e. up to ~1e-7 / alpha^2 at the peak: 2 % at alpha = 0.005. Inherent; bounded in DESIGN.md 10.
 *
 * Glass, ior >= 1 (a value below 1 is taken as written: the outside is then the denser side):
 *   sample (e3):  i = -wo, c = n.i.  c > 0: leaving the medium, n1 = ior, n2 = 1, the normal flips;
 *       otherwise (c = 0, a tangent wo, included) entering, n1 = 1, n2 = ior, cos_i = -c.
 *       cos_t2 = 1 - (n1/n2)^2 (1 - cos_i^2), computed as (1 - (n1/n2)^2) + (n1/n2)^2 cos_i^2 so that a
 *       grazing cos_i is not lost in 1 - cos_i^2.  cos_t2 < 0: total internal reflection, the mirror
 *       direction with probability 1. Otherwise R = R0 + (1 - R0) (1 - x)^5, R0 = ((n1 - n2) / (n1 + n2))^2,
 *       x = cos_i where n1 <= n2, else cos_t = sqrt (cos_t2);  e3 < R reflects with probability R, else
 *       refracts along normalize ((n1/n2 cos_i - cos_t) N + (n1/n2) i) with probability 1 - R (N the
 *       flipped normal). ior = 1 gives R0 = 0 and refraction along -wo.
 *       The direction and the probability are left in the scratch slots.
 *   pdf / eval (wi): a delta lobe. Where the scratch probability is > 0 and wi equals the scratch
 *       direction bit for bit: pdf = that probability, eval = tint * probability / (n.wi), so that
 *       eval (n.wi) / pdf is the tint; 0 for any other wi, and eval = 0 where n.wi = 0 exactly (a wo in
 *       the surface's plane, a refraction at exactly the critical angle): that path dies. */
#define TERRA_GGX_F0        0
#define TERRA_GGX_ROUGHNESS 1
#define TERRA_GGX_END       2
void terra_bsdf_ggx_init ( TerraBSDF* bsdf );

#define TERRA_GLASS_TINT        0
#define TERRA_GLASS_UNUSED      1
#define TERRA_GLASS_SAMPLE_DIR  2
#define TERRA_GLASS_SAMPLE_PROB 3
#define TERRA_GLASS_END         4
void terra_bsdf_glass_init ( TerraBSDF* bsdf );

#define TERRA_DISNEY_BASE_COLOR 0
#define TERRA_DISNEY_SHEEN      1

typedef struct {
    TerraFloat3 base_color;
    float specular, specular_tint;
    float sheen, sheen_tint;
    float clearcoat, clearcoat_gloss;
    float metalness, roughness;
    float anisotropic, subsurface;
} TerraMaterialDisney;

/* Profiler target ids kept for source compatibility; profiling is done with
   rocprofv3 and terra_amd_get_stats() instead (reference include/TerraPresets.h:53-60). */
#define TERRA_PROFILE_SESSION_DEFAULT 0
#define TERRA_PROFILE_TARGET_RENDER   0
#define TERRA_PROFILE_TARGET_TRACE    1
#define TERRA_PROFILE_TARGET_RAY      2
#define TERRA_PROFILE_TARGET_RAY_TRIANGLE_INTERSECTION 3
#define TERRA_PROFILE_TARGET_COUNT    4

#ifdef __cplusplus
}
#endif
#endif /* TERRA_AMD_TERRA_PRESETS_H */
