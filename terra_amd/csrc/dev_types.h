// dev_types.h -- plain-data layouts shared by the host side (scene_host.cpp) and
// the HIP kernels. Everything here is what actually sits in HBM / kernarg.
//
// HBM layout of a committed scene (one replica per GPU):
//   nodes   : DevNode[n_nodes]     64 B each, same size as the reference node
//             (reference src/TerraBVH.h:13-17) but with the two children packed as
//             4 x 16-byte quads so a lane fetches a node with four dwordx4 loads.
//   tris    : DevTri[n_tris]       48 B each: 36 B of vertex data (reference
//             include/Terra.h:109-113) + the (object, triangle) reference in the
//             pad lanes, so a leaf test is three aligned dwordx4 loads.
//   props   : DevProps[n_tris]     64 B each: 60 B of vertex normals/texcoords
//             (reference include/Terra.h:115-122) + 4 B pad.
//   mats    : DevMaterial[n_objects]
//   lights  : DevLight[n_lights], tri_area : float[n_tris] (only light triangles are read)
// The "algorithmic bytes" of the roofline use the reference sizes (64/36/60),
// not the padded ones (DESIGN.md "Roofline").
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <hip/hip_vector_types.h>     // float4 (DevRenderParams::partials)

#define TERRA_DEV_MAX_ATTR 8

struct DevF3 { float x, y, z; };
struct DevF4 { float x, y, z, w; };

// child word: bit 31 clear -> inner node index; bit 31 set -> leaf, low 31 bits = global triangle index;
// 0xFFFFFFFF -> empty slot (only in scenes with < 2 triangles)
#define DEV_CHILD_LEAF  0x80000000u
#define DEV_CHILD_EMPTY 0xFFFFFFFFu

struct DevNode {
    // q0 = min0.xyz, max0.x   q1 = max0.yz, min1.xy   q2 = min1.z, max1.xyz   q3 = child0, child1, prim0, prim1
    // prim = reference leaf index (object | triangle << 8), kept so results carry the reference's TerraPrimitiveRef
    float    min0[3], max0[3];
    float    min1[3], max1[3];
    uint32_t child[2];
    uint32_t prim[2];
};
static_assert ( sizeof ( DevNode ) == 64, "DevNode must be 64 bytes" );

// A fast-tree node as the kernels read it (traverse_fast.h "MODE 2"), 128 bytes = one cache line, FOUR children: per child and axis the two planes of the child's box
// as binary16 rounded outward (min down, max up), times DevScene's power-of-two scale, as one 32-bit word -- the four children's words of an axis side by side and
// every such 16-byte group twice: q[axis][0][child] = min | max << 16 for rays travelling in the axis' positive direction, q[axis][1][child] = max | min << 16 for the
// others, so that a ray LOADS the group whose low half is its near plane (no per-box swap) --, then the four child words (inner: index of a wide node; leaf:
// DEV_CHILD_LEAF | (count - 1) << 27 | first triangle; DEV_CHILD_EMPTY with an inverted box -- min = +65504, max = -65504 -- for a slot not in use). A ray reads four
// 16-byte pieces of a node (its three groups and the child words). Made on the host from the builders' binary tree (tree_build.cpp fastbvh::widen).
struct DevFastNode {
    uint32_t q[3][2][4];
    uint32_t child[4];
    uint32_t pad[4];
};
static_assert ( sizeof ( DevFastNode ) == 128, "DevFastNode must be 128 bytes" );

struct DevTri {
    float    a[3]; uint32_t object;
    float    b[3]; uint32_t tri_in_object;
    float    c[3]; uint32_t pad;
};
static_assert ( sizeof ( DevTri ) == 48, "DevTri must be 48 bytes" );

struct DevProps {
    float na[3], nb[3], nc[3];
    float ta[2], tb[2], tc[2];
    float pad;
};
static_assert ( sizeof ( DevProps ) == 64, "DevProps must be 64 bytes" );

enum DevBsdfKind { kDevBsdfDiffuse = 0, kDevBsdfPhong = 1, kDevBsdfGGX = 2, kDevBsdfGlass = 3 };

// A texture as the reference samples it (reference src/Terra.c:368-466): texel-space lookups,
// 1-byte (x/255) or float components, point or bilinear filter, wrap / mirror / clamp addressing.
struct DevTexture {
    const void* data;              // HBM copy of TerraTexture::pixels (+ 2 elements of padding)
    uint32_t width, height;
    uint32_t components;
    uint32_t depth;                // 1 or 4 bytes per component
    uint32_t filter;               // TerraFilter
    uint32_t address_mode;         // TerraTextureAddressMode
};

struct DevMaterial {
    int32_t  bsdf;                 // DevBsdfKind
    uint32_t attributes_count;
    float    ior;
    uint32_t first_tri;            // offset of the object's triangles in the soup
    float    emissive[3];
    uint32_t tri_count;
    float    attributes[TERRA_DEV_MAX_ATTR][3];
    // texture index per attribute slot (slot TERRA_DEV_MAX_ATTR = emissive), -1 = the constant above
    int32_t  tex[TERRA_DEV_MAX_ATTR + 1];
    int32_t  any_texture;
};

struct DevReplay {                 // one level of the reachability replay (DevScene::ref_replay)
    float    bmin[3];
    uint32_t parent;
    float    bmax[3];
    uint32_t pad;
};

struct DevLight {
    uint32_t object;
    uint32_t first_tri;
    uint32_t tri_count;
    float    area;
};

// One entry of a scene's leaf-box table (scene_host.cpp leaf_box_table; traverse_ref.h "Flat leaf-box test"): a box that one or more leaf children of the
// reference tree carry, bit for bit, and the rank bits (1 << DevTri::pad) of those children's triangles
struct DevLeafBox { float bmin[3], bmax[3]; uint32_t mask; };
static_assert ( sizeof ( DevLeafBox ) == 28, "DevLeafBox must be 28 bytes" );
// leaf-box table: where a ranked launch stages it in LDS (traverse_ref.h "Flat leaf-box test")
#define TERRA_RANKED_ENTRY_BYTES 48                                  // a ranked triangle entry: three 16-byte pieces, the last one c[kz] triangle - -
#define TERRA_RANKED_PAD_OFFSET 40                                   // ... whose two pad words are its last 8 bytes
#define TERRA_LEAF_BOX_STRIDE ( 6 * TERRA_RANKED_ENTRY_BYTES )       // a leaf box: the pad words of six consecutive entries (3 axes x 2 signs)
#define TERRA_LEAF_BOX_MASK_OFFSET 60                                // DevProps::pad in the staged properties of triangle k ...
#define TERRA_LEAF_BOX_MASK_STRIDE 64                                // ... one DevProps per box
static_assert ( TERRA_RANKED_PAD_OFFSET == TERRA_RANKED_ENTRY_BYTES - 8 && TERRA_LEAF_BOX_STRIDE == 288, "leaf-box slots = the last two words of the 48-byte ranked entries" );
static_assert ( offsetof ( DevProps, pad ) == TERRA_LEAF_BOX_MASK_OFFSET && sizeof ( DevProps ) == TERRA_LEAF_BOX_MASK_STRIDE, "leaf-box masks = DevProps::pad of the staged properties" );
// where the table lies, in bytes: the (near, far) pair of box k on axis a for a ray whose direction there is positive (s = 0) or negative (s = 1), from the first
// ranked entry (Tracer::l_ranked); box k's mask, from the first staged DevProps (Tracer::l_props). leaf_boxes_flat reads through these, make_tracer's stores are tied
// to them by static_asserts, terra_amd_leaf_box_offsets (scene_host.cpp) reports them.
constexpr uint32_t terra_leaf_box_plane_offset ( uint32_t k, uint32_t a, uint32_t s ) { return TERRA_LEAF_BOX_STRIDE * k + TERRA_RANKED_ENTRY_BYTES * ( 2u * a + s ) + TERRA_RANKED_PAD_OFFSET; }
constexpr uint32_t terra_leaf_box_mask_offset ( uint32_t k ) { return TERRA_LEAF_BOX_MASK_STRIDE * k + TERRA_LEAF_BOX_MASK_OFFSET; }
#define TERRA_LEAF_BOX_REACH 65535u      // a ds_read's immediate offset is 16 bits: every plane pair of a full table is an immediate away from box 0's
#define TERRA_LEAF_RANK_MAX 32     // triangles a ranked launch can have: a lane's leaf set is one 32-bit word
static_assert ( terra_leaf_box_plane_offset ( TERRA_LEAF_RANK_MAX - 1, 2, 1 ) + 8u - terra_leaf_box_plane_offset ( 0, 0, 0 ) <= TERRA_LEAF_BOX_REACH, "a full leaf-box table within the reach of one base register" );
// pair form of a ranked launch (traverse_ref.h "Pair form"; scene_host.cpp leaf_pair_table): every triangle of the scene is one half of a fan (a, b, c), (a, c, d) inside one
// distinct leaf box. One entry of the commit's table: the two triangles (soup indices, T1 = (a, b, c) first) and their reference visit ranks
struct DevLeafPair { uint32_t tri[2]; uint32_t rank[2]; };
static_assert ( sizeof ( DevLeafPair ) == 16, "DevLeafPair must be 16 bytes" );
// what DevRenderParams::leaf_pairs points at, in 32-bit words, for a scene of n triangles (n / 2 entries): [n / 2 DevLeafPair] [n words: the entry of soup triangle i]
// [one word per distinct leaf box: its mask in ENTRY bits (bit e = entry e), the image of DevLeafBox::mask]
constexpr uint32_t terra_leaf_pair_words_entry_of ( uint32_t n_tris ) { return 2u * n_tris; }
constexpr uint32_t terra_leaf_pair_words_masks ( uint32_t n_tris ) { return 3u * n_tris; }
// where a pair launch stages its section in LDS, in place of the ranked entries (Tracer::l_ranked): 6 permuted copies x n / 2 entries x 64 B (p0 p1 p2 p3 in (kx, ky, kz), then
// the two record keys and two spare words), then the leaf-box table in a part of its own -- 48 B per box, axis major, both signs: box k's (near, far) pair on axis a for
// direction sign s at 48 k + 8 (2 a + s) -- so that a group of eight boxes is still read at immediate offsets (box 7 at 336 B). The masks stay where the single form has them.
#define TERRA_PAIR_ENTRY_BYTES 64
#define TERRA_PAIR_BOX_STRIDE 48
constexpr uint32_t terra_pair_entry_offset ( uint32_t n_pairs, uint32_t perm, uint32_t e ) { return TERRA_PAIR_ENTRY_BYTES * ( perm * n_pairs + e ); }
constexpr uint32_t terra_pair_boxes_offset ( uint32_t n_pairs ) { return 6u * TERRA_PAIR_ENTRY_BYTES * n_pairs; }
constexpr uint32_t terra_pair_box_plane_offset ( uint32_t k, uint32_t a, uint32_t s ) { return TERRA_PAIR_BOX_STRIDE * k + 8u * ( 2u * a + s ); }
constexpr uint32_t terra_pair_section_bytes ( uint32_t n_pairs ) { return terra_pair_boxes_offset ( n_pairs ) + TERRA_PAIR_BOX_STRIDE * n_pairs; }
static_assert ( terra_pair_box_plane_offset ( 7, 0, 0 ) == 336 && terra_pair_box_plane_offset ( 0, 2, 1 ) + 8u == TERRA_PAIR_BOX_STRIDE, "a box = six 8-byte plane pairs; a group of eight within 384 bytes" );
// shading constants (make_tracer fills, surface_init<1> reads): 48 bytes per staged triangle of a PAIR-FORM launch, behind the pair section --
// e0[3], e1[3], d00, d11, d01, div = d00 d11 - d01 d01, rcp_exact ( div ), and a flag word: 1 where div is inside the range in which the short quotient form is
// valid (exact_div.h xd_rcp_ok: normal, 2^-60 <= |div| <= 2^60, significand not all ones), 0 for a zero, denormal, non-finite or out-of-range div.
// Only pair-form launches have it: a pair section is 216 bytes per triangle where the ranked entries the plan budgeted are 288, so section + constants (264) never
// take more LDS than the plan allowed and resident_leaf_cap stays as it is. Cornell: 29,456 + 32 x 48 = 30,992 B <= TERRA_LDS_BUDGET.
// Every launch without the pair form stages nothing and surface_init computes the constants per hit. The A/B of both: profiles/exact_div/ab.md.
#define TERRA_SHADE_CONSTS_BYTES 48u
static_assert ( terra_pair_section_bytes ( TERRA_LEAF_RANK_MAX / 2 ) + TERRA_SHADE_CONSTS_BYTES * TERRA_LEAF_RANK_MAX <= 6u * TERRA_RANKED_ENTRY_BYTES * TERRA_LEAF_RANK_MAX
                && terra_pair_section_bytes ( 1 ) + TERRA_SHADE_CONSTS_BYTES * 2u <= 6u * TERRA_RANKED_ENTRY_BYTES * 2u, "pair section + shading constants fit where the plan budgeted ranked entries" );
static_assert ( terra_pair_section_bytes ( TERRA_LEAF_RANK_MAX / 2 ) <= 6u * TERRA_RANKED_ENTRY_BYTES * TERRA_LEAF_RANK_MAX && terra_pair_section_bytes ( 1 ) <= 6u * TERRA_RANKED_ENTRY_BYTES * 2u, "the pair section never takes more LDS than the ranked entries it replaces" );
#define TERRA_LEAF_PAIRS_NEAREST 1u          // DevRenderParams::leaf_pairs, lowest bit: nearest first (the distance itself is a multiple of 4)
// a record key of the pair loop: (rank + 1) << 5 | soup triangle -- ordered as the ranks are, 0 = no hit, the triangle in its low five bits
constexpr uint32_t terra_pair_key ( uint32_t rank, uint32_t tri ) { return ( rank + 1u ) << 5 | tri; }
static_assert ( TERRA_LEAF_RANK_MAX <= 32, "a pair key keeps the triangle in five bits" );
// launch plan: the constants both the host's plan (launch_plan.h) and the device code read
#define TERRA_LEAF_CAP_MAX 16
#define TERRA_COL 256              // stride of a stack / leaf-list column: the block's thread count
#define TERRA_LDS_NODE_BYTES 112   // staged node (traverse_ref.h "Staged node")
// per-thread words parked in LDS between uses (indexed [word][thread] like the stack): the radiance sum of the lane's
// current job (touched once per path), the job's number and the lane's draw count when the job started (read at its end), and a row
// that holds each wave's pool of claimed jobs (render_kernels.hip "jobs")
#define TERRA_AUX_WORDS 6        // rows every launch has (acc x 3, job, draw count, wave pools)
#define TERRA_AUX_WORDS_LDS 9    // ... plus, on LDS-resident scenes (lds_mode 1), the path radiance Lo x 3 (render_kernels.hip LO_LDS)
#ifndef TERRA_FAST_STACK_LDS     // entries of a fast-tree launch's stack kept in LDS, the rest in HBM (launch_plan.h terra_plan_fast_tree)
#define TERRA_FAST_STACK_LDS 16
#endif
#ifndef TERRA_LDS_CU_KB
#define TERRA_LDS_CU_KB 158
#endif
#ifndef TERRA_LEAF_CAP_MIN       // smallest leaf list worth an extra resident block (with the decoupled loop, hall: 5 blocks x 6 entries
#define TERRA_LEAF_CAP_MIN 6     // 391 ms vs 4 blocks x 14 entries 400 ms, Direct 473 vs 487 ms; profiles/r01_measurements/ab_lc*.log)
#endif
#ifndef TERRA_LDS_BUDGET          // per block, so that FIVE blocks stay resident per CU: a CU does not hand out all of its 160 KB -- 5 x 31,632 B fit, 5 x 32,656 B
#define TERRA_LDS_BUDGET ( TERRA_LDS_CU_KB * 1024 / 5 )      // do not (measured: 4.57 -> 3.67 waves per SIMD and 65.6 -> 74.4 ms on the Cornell frame, profiles/r03_measurements/lds_cliff.log)
#endif
#ifndef TERRA_LEAF_CAP_RESIDENT_MIN
#define TERRA_LEAF_CAP_RESIDENT_MIN 8
#endif
#ifndef TERRA_LDS_BLOCK_MAX_KB      // the most dynamic LDS one block may opt in to (a CU's 160 KB less what the runtime keeps)
#define TERRA_LDS_BLOCK_MAX_KB 156
#endif
#ifndef TERRA_JOB_ORDER_MIN_BLOCKS
#define TERRA_JOB_ORDER_MIN_BLOCKS 256
#endif

struct DevScene {
    const DevNode*     nodes;
    const DevTri*      tris;
    const DevProps*    props;
    const DevMaterial* mats;
    const DevLight*    lights;
    const float*       tri_area;
    const DevTexture*  textures;
    uint32_t n_nodes, n_tris, n_objects, n_lights;
    uint32_t lights_triangles_count;
    int32_t  max_stack;
    // optional second accelerator over the same triangles (terra_amd_set_tree_mode, DESIGN.md "Fast tree"):
    // 3-axis binned-SAH BVH2, leaves of up to 4 triangles; fast_tris is the soup in leaf order with
    // DevTri::pad = the triangle's rank in the REFERENCE tree's leaf visit order (the tie-break key)
    const DevNode*     fast_nodes;      // the device builder's output: a binary tree with (min, max) boxes (read back, checked and widened by the host; nullptr for host-built trees)
    const DevFastNode* fast_nodes_h;    // the tree as traversed: 4-wide nodes of binary16 planes (tree_build.cpp fastbvh::widen)
    const DevTri*      fast_tris;
    uint32_t n_fast_nodes;              // wide nodes
    int32_t  fast_max_stack;            // stack entries a ray can need in the wide tree
    float    fast_inv_scale;            // 1 / (the power of two DevFastNode's planes are stored times): the factor of the ray's inverse direction
    // scenes outside the coordinate range of the containment proof (DESIGN.md "Reachability"): the fast tree (boxes inflated to the rounding bound) finds the
    // candidates, and one is accepted only if the REFERENCE traversal would have reached it, i.e. if the slab tests of its ancestors in the reference tree pass.
    // ref_replay[q] (DevReplay, 32 B) = the box the reference tests before it visits inner node q -- stored in q's parent -- and that parent's index, so that one
    // 32-byte fetch gives a level's test AND the way up (node 0 = the root: never tested); fast_leaf_parent[i] = the reference node whose leaf child fast triangle i is
    const struct DevReplay* ref_replay;
    const uint32_t*    fast_leaf_parent;
    // fast_leaf_mask[i]: bit L set = the slab test of the L-th node on the way up from fast triangle i's leaf (L = 0: the leaf's node) has to be replayed for a ray that
    // hits the triangle. A clear bit = it cannot fail: either the box contains the triangle's extent with a clearance above the rounding bound (the containment
    // argument, at the scene's scale), or it contains the box of level L - 1 component by component -- then, for a ray whose inverse direction is finite and non-zero,
    // (b - o) * inv being monotone in b makes "level L - 1 passes" imply "level L passes" in the very same float arithmetic. Rays that are not regular replay every
    // level. Bit 31 stands for every level from 31 up.
    const uint32_t*    fast_leaf_mask;
    uint32_t           reach;
    // (cos, sin) of 2 * terra_PI * (k * 2^-24) for k = 0 .. 2^24 - 1: the azimuth the BSDF samplers make of a stream-B variate, tabulated once per device
    // (128 MB of HBM; shading_device.h azimuth_fetch). nullptr (the default) = compute.
    const float2*      sincos24;
    // environment lighting (terra_amd_set_environment_lighting; off = the reference's behaviour):
    // 0 off, 1 constant env_color, 2 lat-long lookup of textures[env_tex] by ray direction
    int32_t  env_mode;
    int32_t  env_tex;
    float    env_color[3];
    // environment importance sampling (terra_amd_set_environment_sampling; compiled into the KINDS & TERRA_KIND_SAMPLER variants only): the lat-long map textures[env_tex]
    // as a TerraDistribution2D (reference src/Terra.c:812-846) over luminance x sin(theta of the row): env_f / env_cdf = the env_nx x env_ny table and each row's
    // normalised running sum, env_row_f / env_row_cdf = the rows' totals and their normalised running sum, env_integral = the total. env_nx == 0: off.
    const float* env_f; const float* env_cdf; const float* env_row_f; const float* env_row_cdf;
    uint32_t env_nx, env_ny; float env_integral; uint32_t env_monotone;
};
// bit of the kernels' KINDS mask (bits 0-3 = DevBsdfKind present) that compiles the environment term in
#define TERRA_KIND_ENV 16
// ... and the bit that compiles textured-attribute sampling into terra_surface_init's counterpart
#define TERRA_KIND_TEX 32
// ... and the bit that compiles the sampler integration in (terra_amd_set_sampler_integration: the pixel's Halton / stratified sampler feeds the first bounce)
#define TERRA_KIND_SAMPLER 64
// ... and the bit that compiles environment MIS in (terra_amd_set_environment_mis: Direct + MIS weights its environment sample against its BSDF ray). A launch
// parameter: fill_params sets it in DevRenderParams::bsdf_kinds, next to TERRA_KIND_SAMPLER, only where it acts; it selects a variant of its own, so the sampler
// variant every other environment-sampling render runs is the code it was without it
#define TERRA_KIND_ENV_MIS 128

// indices into the device counter array (uint64 each); mirrors TerraAmdStats
enum { kCtrRays = 0, kCtrNodes, kCtrBoxTests, kCtrTriTests, kCtrHits, kCtrSamples, kCtrRandCalls, kCtrAttrFetches, kCtrPixels, kCtrLaunches, kCtrFaults, kCtrTriCulled,
       kCtrDbg0, kCtrDbgLast = kCtrDbg0 + 15, kCtrSkipProved /* not part of TerraAmdStats; stored, not counted: the blocks the last launch proved empty (terra_amd_empty_skip_info; zeroed with the counters by terra_amd_reset_stats) */, kCtrCount };   // kCtrFaults: only written by TERRA_CHECK_BOUNDS builds; kCtrDbg*: only by TERRA_PHASE_STATS builds (lane-occupancy study)

struct DevRenderParams {
    DevScene scene;
    // camera (reference src/Terra.c:1770-1799): rot rows, position, tan(fov/2) (host double tan, rounded), aspect
    float    cam_rot[9];
    float    cam_pos[3];
    float    tan_half_fov;
    float    aspect;
    float    jitter;
    float    exposure;
    float    gamma;
    uint32_t fb_w, fb_h;
    uint32_t x, y, w, h;            // rectangle to render
    // where pixel (px, py) of the frame lives in `pixels` / `results` / `rand_calls`: element (py - st_y) * st_pitch + (px - st_x).
    // Device-resident frames: st_x = st_y = 0, st_pitch = fb_w; terra_render() on a host frame stages the rectangle only.
    uint32_t st_x, st_y, st_pitch;
    uint32_t tile_size, rank, world; // sharding: tiles t with t % world == rank (world == 1: everything)
    uint32_t spp;                   // effective samples per pixel (after the stratified round-up)
    // sample split (terra_amd_set_sample_split): the call's spp samples are cut into `split` = 2^split_log2 chunks
    // of chunk_spp, one lane per (pixel, chunk); chunk j draws from the streams keyed (pixel, samples_so_far + j*chunk_spp)
    // and its radiance sum goes to partials[(j * blocks + block) * 256 + thread] = {sum.xyz, rand calls};
    // terra_resolve_kernel then adds the chunk sums to the pixel IN CHUNK ORDER -- exactly what `split`
    // successive calls of chunk_spp samples produce. split == 1: one chunk, the call's own sum (src/Terra.c:551-572).
    uint32_t split, split_log2, chunk_spp;
    float4*  partials;
    // job_streams[2 * job], [2 * job + 1]: the random streams of job `job`, keyed ahead of the render kernel by terra_job_streams_kernel with every lane busy -- {A.state, B.state},
    // {B.inc, px | py << 16 (all ones: a pixel outside the rectangle), samples already in the pixel} -- so that a lane at a job boundary loads 32 bytes instead of hashing its keys (ten 64-bit multiplications) nearly alone
    uint4*   job_streams;
    // job space of the persistent render grid (render_kernels.hip "jobs"): job_blocks virtual 256-thread blocks = (16x16 pixel blocks of the
    // shard) * split; *job_queue (zeroed before the launch) hands out the jobs beyond the ones the launched lanes start with
    uint32_t job_blocks;
    uint32_t* job_queue;
    // job order (launches that key their streams ahead, render_kernels.hip "job order"): the 16x16 pixel blocks of the launch are handed out in the order
    // block_order[0 .. blocks) -- the blocks some camera ray hits first, the blocks whose camera rays all leave the scene last, so that the launch ends on short jobs --
    // and block_order[blocks + b] is where pixel block b went (the resolve kernel finds the block's sums there). nullptr: the order of the numbering.
    const uint32_t* block_order;
    // the job decode's divisions by launch constants as multiplications: ceil(2^32 / d) (0 for d == 1) for d = (blocks per tile)^2, tiles per row of the
    // rectangle, blocks per tile row (the host refuses a launch in which some product n * d could reach 2^32)
    uint32_t job_div_bpt2, job_div_tiles_x, job_div_bpt, job_tiles_x;
    uint32_t bounces;
    int32_t  integrator;
    int32_t  tonemap;
    uint64_t frame_seed;
    float*   pixels;                // 3 floats per pixel
    void*    results;               // {float acc[3]; int samples} per pixel
    uint32_t* rand_calls;           // optional
    unsigned long long* counters;   // kCtrCount entries
    // LDS plan of a block (host decides -- launch_plan.h --, kernel obeys): stack_depth stack entries per thread,
    // lds_nodes nodes (breadth-first prefix) and lds_tris triangles (+ their vertex properties)
    // staged; leaf_cap deferred-leaf entries per thread; lds_mode 0 = nothing staged, 1 = whole scene
    uint32_t stack_depth, leaf_cap, lds_nodes, lds_tris;
    // fast-tree launches: entries of a lane's traversal stack beyond the stack_depth kept in LDS live in HBM -- stack_spill[(resident lane) * spill_cap + (entry - stack_depth)]
    // (the launch's scratch; nullptr when the whole stack fits in LDS). Rarely touched: the LDS part covers the depth a ray actually reaches, the bound is the tree's worst case.
    uint32_t* stack_spill; uint32_t spill_cap;
    int32_t  lds_mode;
    int32_t  count_level;           // work counters: 0 none (the default), 2 all six per lane (terra_amd_set_work_counters, or a per-pixel draw-count buffer was passed)
    uint32_t bsdf_kinds;            // mask of DevBsdfKind present in the scene (bit k = kind k)
    uint32_t leaf_cull;             // 1: skip the triangle test of a leaf child whose box the ray misses (Tracer::cull); host decides per call
    uint32_t fused_slab;            // 1: a cull launch inside the coordinate range: inner boxes may be decided with the fused slab arithmetic (Tracer::fused)
    uint32_t leaf_rank;             // 1: an LDS-resident launch of at most TERRA_LEAF_RANK_MAX triangles: leaves collected as a set of reference visit ranks (Tracer::ranked)
    // sampler integration (terra_amd_set_sampler_integration; compiled into the KINDS & TERRA_KIND_SAMPLER variants only): 0 off, 1 Halton, 2 stratified
    // (`sampler_strata` strata per dimension, 16 samples per stratum: the sampler the reference constructs at src/Terra.c:542)
    uint32_t sampler_mode, sampler_strata;
    // shading stages (exact_div.h "Shading stages"; the kernels of trace_geometry.h ray_start_masks_for): 1 = the launch's camera lies outside the limits for which
    // the first stage may leave out range tests (terra_camera_stage_limits below), and it takes the guarded ray start, every site with its own test. fill_camera
    // decides once per launch. (A 32-bit word in what was padding before job_live: the structure keeps its size and every field its offset.)
    uint32_t shade_s1_guarded;
    // empty skip (render_kernels.hip "proved empty"): the job order ends with the blocks that empty_proof.h proved empty; *job_live = the jobs before them
    // (live blocks x split x 256, written by terra_block_order_kernel). Those blocks are never keyed, queued or traced: the resolve kernel adds their +0 sums.
    // nullptr: every block is live. (Last, so that the kernels that never read it keep their argument offsets.)
    const uint32_t* job_live;
    // flat leaf-box test (traverse_ref.h "Flat leaf-box test"; terra_amd_set_leaf_box_test): n_leaf_boxes > 0 = a ranked fused launch without work counters stages the
    // scene's table of distinct leaf boxes (leaf_boxes: n_leaf_boxes entries in the scene blob) and its tame waves test those boxes instead of walking the tree
    const DevLeafBox* leaf_boxes;
    uint32_t n_leaf_boxes;
    // pair form (traverse_ref.h "Pair form"; terra_amd_set_leaf_pairs): non-null = a ranked launch without work counters of a scene in which every triangle is half of a
    // fan inside one leaf box stages the pairs (dev_types.h "pair form": the table in the scene blob) and its leaf loop tests both triangles of a pair in one trip.
    // The table's distance in bytes from scene.tris, inside the same blob; 0 = none. (A 32-bit word in what was padding: the structure keeps its size, so the kernels
    // that never read it keep their argument offsets.)
    // Nearest first (traverse_ref.h "Nearest first"; terra_amd_set_leaf_nearest_first): the table is 4-byte aligned in the blob, so the distance's lowest bit is free:
    // TERRA_LEAF_PAIRS_NEAREST set = the launch's flat lanes test their nearest box's entry first and drop the entries beyond the record. The host sets it only beside a
    // table of distinct leaf boxes in which box k holds exactly entry k.
    uint32_t leaf_pairs;
    // 1.f / (float) fb_w, 1.f / (float) fb_h, correctly rounded on the host (fill_camera): camera_sample's two divisions by the frame size take them through div_exact_rk
    // (exact_div.h). No padding was left: the record grows by 8 bytes, at its end, so every other field -- and the argument offsets of the kernels that read no camera --
    // stays where it was; a ray-sourced launch's ray pointer (DevRayRenderParams) moves 8 bytes up.
    float    inv_fb_w, inv_fb_h;
};
static_assert ( sizeof ( DevRenderParams ) == 576 && offsetof ( DevRenderParams, job_live ) == 544, "shade_s1_guarded sits in padding: no field of the launch parameters moved" );
// The limits of DevRenderParams::shade_s1_guarded, checked once per launch where the camera is filled in (host code; plain C++): aspect * tan_half_fov and
// tan_half_fov in [2^-30, 2^20] and every entry of the rotation of magnitude <= 2 (a NaN fails). Inside them, in trace_geometry.h camera_sample_staged: the film
// vector ( fx, fy, 1 ) has a squared length in [1, 2^41] and a length in [1, 2^21]; fx and fy are 0 or no smaller than 2^-24 * 2^-30 * ( 1 - 2^-22 ) > 2^-60 (a
// film coordinate 2 ndc - 1 is 0 or a multiple of 2^-24 near 0); and a rotated unit direction has components below 6 ( 1 + 2^-20 ).
inline bool terra_camera_stage_limits ( float aspect, float tan_half_fov, const float* rot9 ) {
    const float at = aspect * tan_half_fov;
    bool ok = at >= 0x1p-30f && at <= 0x1p20f && tan_half_fov >= 0x1p-30f && tan_half_fov <= 0x1p20f;
    for ( int i = 0; i < 9; ++i ) ok = ok && ( rot9[i] >= -2.f && rot9[i] <= 2.f );
    return ok;
}
// masked launches (include/terra_amd.h "Masked rendering"; render_kernels.hip "masked launches"): which 16x16 pixel blocks of the rectangle a launch renders. A property
// of the launch, beside its ray source, not a field of DevRenderParams: the small kernels around the render grid take its two pointers as arguments of their own, the
// render kernels that key their streams ahead read DevRenderParams::job_live and the job table as they stand, and so no kernel-argument offset of any kernel moves
// and no render kernel changes (the kernels that key their streams in place cannot be launched masked: scene_host.cpp masked_plan_check).
//   words: ceil(w / 16) * ceil(h / 16) words, row-major in the rectangle (not in the launch's tile-major block numbering), non-zero = active;
//   live_blocks: a word of the launch's scratch header (its own cache line, as job_live's): the blocks the order placed before the masked ones, written by
//   terra_block_order_kernel, read by terra_resolve_kernel -- a block at or beyond it is left alone.
struct DevLaunchMask { const uint32_t* words; uint32_t* live_blocks; };
#define TERRA_CLASS_MASKED 3u      // the block class of an inactive block: the last one (0 hit, 1 empty by probe, 2 proved empty)
// ray-sourced launches (include/terra_amd.h "Ray-sourced rendering"): the launch's parameters end with the ray buffer -- one TerraAmdRay (two 16-byte words) per pixel,
// addressed like `results` (st_x / st_y / st_pitch: the frame for the device forms, the staged rectangle for the host forms). The pointer follows DevRenderParams' last field in a structure of its own, which only
// the ray-sourced kernel instances take: no field of DevRenderParams moves and the camera kernels keep their kernel-argument segment to the byte.
struct DevRayRenderParams : DevRenderParams { const float4* rays; };
// lens launches (include/terra_amd.h "Lens rendering"): the camera model and its constants as fill_lens rounds them on the host; the launch's camera fields
// (cam_pos, cam_rot, aspect, tan_half_fov, jitter, inv_fb_*) are filled as for a camera launch. The generator: lens_sample, trace_geometry.h.
struct DevLens {
    int32_t model;              // 0 perspective (pinhole / thin lens), 1 orthographic, 2 equirectangular, 3 fisheye
    float   lens_radius;        // model 0: aperture radius; 0 = pinhole (no lens pair is drawn)
    float   focus_distance;     // model 0, lens_radius > 0
    float   ortho_half;         // model 1: ortho_height * 0.5f
    float   fisheye_half;       // model 3: (fisheye_fov * 0.0174533f) / 2
};
// ... and their parameters: DevRenderParams followed by the lens, a structure only the lens kernel instances take (as DevRayRenderParams and for its reason)
struct DevLensRenderParams : DevRenderParams { DevLens lens; };
// point launches (include/terra_amd.h "Point rendering"): one TerraAmdPoint (two 16-byte words: {position, -} {normal, -}) per pixel, addressed like `results` as a
// ray-sourced launch's rays are, and the distribution every sample's direction is drawn from about the point's normal. The generator: point_sample, trace_geometry.h.
struct DevPointSampling {
    int32_t distribution;       // 0 cosine-weighted hemisphere about the normal, 1 uniform sphere
};
// ... and their parameters, a structure only the point kernel instances take (as DevRayRenderParams and for its reason)
struct DevPointRenderParams : DevRenderParams { const float4* points; DevPointSampling sampling; };
// Where a launch's primary rays come from, TERRA_RAY_SOURCE: 0 the pinhole camera's sample, 1 the ray buffer (ray-sourced), 2 a camera model's sample (lens),
// 3 a direction drawn about the pixel's point (points).
// Ray-sourced, lens and point kernel instances are units of their own: render_kernels.hip compiled with TERRA_TU 4 - 7 / 8 - 11 / 12 - 15 and aov_kernels.hip with
// TERRA_TU 4 / 8 / 12 (terra_amd/build.py), or with -DTERRA_RAY_SOURCE=1 / 2 / 3 and no TERRA_TU (tools/kernel_resources.sh).
#ifndef TERRA_RAY_SOURCE
#if defined ( TERRA_TU ) && TERRA_TU >= 12
#define TERRA_RAY_SOURCE 3
#elif defined ( TERRA_TU ) && TERRA_TU >= 8
#define TERRA_RAY_SOURCE 2
#elif defined ( TERRA_TU ) && TERRA_TU >= 4
#define TERRA_RAY_SOURCE 1
#else
#define TERRA_RAY_SOURCE 0
#endif
#endif
