// traverse_ref.h -- the reference-order BVH traversal (trace_device.h lists the layers): work counters, the Tracer, the node and leaf
// steps, the ranked traversal of small LDS-resident scenes, the resumable form of the decoupled render loops.
#pragma once
#include "trace_geometry.h"
#include <stddef.h>

// per-lane work counters (registers); flushed with one atomic per wave and counter.
// Not counted on the device because the host can derive them exactly: slab tests
// (= 2*nodes - tri_tests: every child of a popped node is either slab-tested or, if a
// leaf, triangle-tested), camera samples and pixels (tile geometry x spp).
#ifndef TERRA_PHASE_STATS          // lane-occupancy study builds (tools/phase_stats.py): per-phase wave iterations / active lanes
#define TERRA_PHASE_STATS 0
#endif
struct Counters {
    uint32_t rays, nodes, tri_tests, hits, rand_calls, attr_fetches;
    uint32_t tri_culled;     // leaves met whose triangle test was skipped (Tracer::cull); counted at COUNT level 2 only
#if TERRA_PHASE_STATS
    uint32_t ps[16];
#endif
};
TD Counters counters_zero() {
    Counters c; c.rays = c.nodes = c.tri_tests = c.hits = c.rand_calls = c.attr_fetches = c.tri_culled = 0;
#if TERRA_PHASE_STATS
    for ( int i = 0; i < 16; ++i ) c.ps[i] = 0;
#endif
    return c;
}
#if TERRA_PHASE_STATS
// PS_WAVE: +1 per wave (the first active lane counts); PS_LANE: +1 per active lane
#define PS_WAVE(c, k) do { if ( ( int ) ( threadIdx.x & 63 ) == __ffsll ( ( long long ) __ballot ( 1 ) ) - 1 ) ++( c ).ps[k]; } while ( 0 )
#define PS_LANE(c, k) do { ++( c ).ps[k]; } while ( 0 )
#else
#define PS_WAVE(c, k) do { } while ( 0 )
#define PS_LANE(c, k) do { } while ( 0 )
#endif
enum { kPsRayIter = 0, kPsNodeIter, kPsLeafIter, kPsShadeIter, kPsCamIter, kPsCamLanes, kPsRayLanes, kPsShadeLanes, kPsNodeLanes, kPsLeafLanes, kPsDrainIter,
       kPsTop64, kPsTop256, kPsTop1024, kPsTop4096 };      // node visits that fall into the first K nodes of the (breadth-first numbered) array: what an LDS-staged prefix would serve

// -----------------------------------------------------------------------------
// Tracer: where a thread finds the scene and its traversal scratch.
//
// LDS layout of a block (DESIGN.md "LDS"): [staged nodes: lds_nodes x 112 B] [staged triangles: lds_tris x 48 B]
// [staged vertex properties: lds_tris x 64 B] [node stack: stack_depth x 256 ints] [leaf list: leaf_cap x 256 ints]
// [per-thread parked words]. Stack and leaf list are indexed [entry][thread] so the 64 lanes of a wave touch
// 64 consecutive words (conflict free); a lane walks its column with a pointer (one add per push / pop).
// Nodes and triangles are staged only when the whole scene fits.
//
// Staged node (MODE 1), 7 x 16 B, "axis major, both signs":
//     [x+] min0.x max0.x min1.x max1.x     [x-] max0.x min0.x max1.x min1.x
//     [y+] ...                             [y-] ...
//     [z+] ...                             [z-] ...
//     [children] child0 child1 bit0 bit1   (an inner child = the BYTE OFFSET of its staged node, a leaf = DEV_CHILD_LEAF | triangle; bit0 / bit1: see below)
// A ray whose inverse direction is finite and non-zero on every axis reads, per axis, the copy that matches the sign of its
// direction (SlabSel): the four floats are then (near plane, far plane) of child 0 and of child 1, so the slab test needs no
// per-axis min/max at all -- v_min/v_max_f32 issue at 0.57 G/s per SIMD on gfx950 against 0.96 for v_sub/v_mul_f32
// (profiles/r02_measurements/valu_rates.log). Picking the plane by the sign is exactly min(t1, t2) / max(t1, t2): for
// bmin <= bmax, (b - o) * inv is monotone in b (both roundings are), increasing for inv > 0 and decreasing for inv < 0.
//
// Ranked launches (DevRenderParams::leaf_rank: LDS-resident scenes of at most TERRA_LEAF_RANK_MAX triangles, traverse_ranked): bit0 / bit1 of a leaf child =
// 1 << (its triangle's reference visit rank, DevTri::pad), 0 for an inner child or an empty slot (0 in every other launch). The leaf list is replaced by
// the triangles staged in rank order once per axis permutation of the watertight test (kz = the dominant axis, kx / ky swapped when d[kz] < 0):
// 6 copies x lds_tris x 48 B, entry = a[kx] a[ky] a[kz] b[kx] | b[ky] b[kz] c[kx] c[ky] | c[kz] triangle - -.
//
// Flat leaf-box test (DevRenderParams::n_leaf_boxes: ranked launches with the fused box test and no work counters; leaf_boxes_flat). The node loop of a ranked
// launch only computes "which leaf boxes does this ray pass", so the block also stages the scene's DISTINCT leaf boxes (DevLeafBox: the two triangles of an
// axis-aligned quad share one box bit for bit; the Cornell box has 16 for its 32 triangles) and a tame wave tests every one of them in a wave-uniform loop -- no
// stack, no child words, no trip count set by the slowest lane. The table takes NO LDS of its own: a 48-byte-per-box table beside the other sections would put the
// Cornell block (launch_plan.h terra_lds_bytes: 31,760 B) at 32,592 B, past the TERRA_LDS_BUDGET that keeps five blocks per CU resident (DESIGN.md 3.1 "Flat leaf-box test" has
// the arithmetic). It lives in words the ranked layout leaves unused,
//     the two pad words of the ranked triangle entries (the `- -` above): entry 6 k + 2 a + s (counted through the copies) = box k, axis a:
//         (min, max) for s = 0, (max, min) for s = 1 -- "both signs", as the staged node: a ray reads (near, far) of an axis with one 8-byte load from the slot
//         its direction's sign picks (terra_leaf_box_plane_offset ( 0, a, s ) = 48 x (2 a + s) + 40, formed once per traversal), box k at the immediate offset 288 k;
//     the pad word of the staged vertex properties of triangle k (DevProps::pad): the rank mask of box k.
// A scene has at most as many distinct leaf boxes as triangles, so 6 boxes-worth of entries and one mask word per box are always there.
//
// Pair form (DevRenderParams::leaf_pairs: ranked launches without work counters of a scene whose every triangle is one half of a fan (a, b, c), (a, c, d) inside one
// distinct leaf box -- the two triangles of a quad; scene_host.cpp leaf_pair_table; traverse_pairs). A lane that passes a leaf box tests both of its triangles, so the
// leaf set is a set of ENTRIES (bit e = pair e, in the staged nodes' bit0 / bit1 and in the leaf-box masks alike) and one trip of the leaf loop tests a pair: the
// four vertices are transformed once, the diagonal's edge function is computed once, and the determinant / depth / division part runs once for the triangle that
// passed its sign test (watertight_pair). The ranked entries give way to 6 permuted copies x pairs x 64 B,
//     entry = p0[kx] p0[ky] p0[kz] p1[kx] | p1[ky] p1[kz] p2[kx] p2[ky] | p2[kz] p3[kx] p3[ky] p3[kz] | key of T1, key of T2, - -     (T1 = p0 p1 p2, T2 = p0 p2 p3),
// followed by the leaf-box table in a part of its own (dev_types.h "pair form": 48 B per box). A pair tested because only its partner's leaf was reached on a walk is
// harmless for the reason given under "Flat leaf-box test": a triangle whose box the ray misses is not hit.
// -----------------------------------------------------------------------------
// (the table's constants and byte offsets: dev_types.h "leaf-box table", shared with the host; TERRA_LEAF_CAP_MAX, TERRA_COL, TERRA_LDS_NODE_BYTES: dev_types.h "launch plan")
#define TERRA_LEAF_BOX_GROUP 8     // boxes per trip of the unrolled loop (offsets as immediates); four left over are one trip more, the up to three boxes after that are tested one per trip

struct Tracer {
    DevScene      sc;
    const float4* l_nodes;     // LDS copies (valid for index < lds_nodes / lds_tris)
    const float*  l_tris;
    const float4* l_props;
    const DevMaterial* l_mats;  // materials, lights, per-triangle areas: the block's LDS copies in MODE 1, the arrays in HBM otherwise (make_tracer)
    const DevLight*    l_lights;
    const float*       l_area;
    const float4* l_ranked;    // ranked launches: the 6 permuted copies of the staged triangles, in rank order -- pair form: the pair section, 6 copies of the entries then the leaf-box table -- (see above); nullptr otherwise
    const float4* l_consts = nullptr;      // pair-form launches: three float4 per staged triangle (dev_types.h "shading constants"); nullptr in every other launch and in every Tracer filled by hand
    uint32_t      n_boxes;     // flat leaf-box test: the distinct leaf boxes staged -- planes in the pad words of l_ranked (pair form: in the pair section's own part), masks in those of l_props (see above); 0 in every other launch
    uint32_t      lds_nodes, lds_tris;
    int*          stack;       // this thread's column
    int*          leaves;
    int           leaf_cap;    // entries in the leaf list (>= 2)
    int           stack_cap;   // entries in the stack column (TERRA_CHECK_BOUNDS builds verify every push against it)
    // fast-tree launches: entries beyond the LDS column live in HBM (DevRenderParams::stack_spill): spill = this lane's spill_cap words, nullptr when the column holds the whole stack
    uint32_t      stack_lim;   // 32-bit LDS address of the block's stack words + stack entries * 1024: wave-uniform (fast_push / fast_pop)
    uint32_t*     spill;
    uint32_t      spill_cap;
    unsigned long long* faults;
    // leaf-box cull (DESIGN.md "Leaf-box cull"): a leaf child's triangle is tested only if the ray passes the slab test of
    // that child's box -- the box the node already carries and the node step already tests. The reference tests the triangle
    // unconditionally (src/TerraBVH.c:284-300); the closest hit is the same whenever a triangle the ray hits lies inside its
    // own +-1e-4 box as the slab test sees it, which the host verifies numerically at commit (terra_cull_margin_ok).
    bool cull;
    // cull launches INSIDE the coordinate range may also decide the inner boxes with the fused slab arithmetic (slab_near_far_fused): the containment proof covers
    // every box there. Outside it (Scene::reach_cull) only the rebuilt leaf boxes carry a margin; the inner boxes must be tested exactly as the reference tests them.
    bool fused;
    // the leaves a ray meets are collected as a set of ranks in one register instead of a list in LDS (traverse_ranked); launch constant
    bool ranked;
    // ... and the ranked entries are pairs (see "Pair form" above); launch constant, only ever set in launches without work counters
    bool pairs;
    // ... and a lane of a flat pair-form launch tests the entry of its nearest box first and drops the entries beyond the record (traverse_pairs "Nearest first";
    // terra_amd_set_leaf_nearest_first); launch constant, only ever set where box k holds exactly entry k
    bool nearest = false;
};
// The Tracer of a launch that stages nothing (the AOV, query and unit kernels): the scene read from HBM; words = the block's stack_depth stack entries, then leaf_cap
// leaf-list entries, each 256 ints; spill = the HBM part of the launch's fast-tree stacks, spill_cap words per lane of the grid, lane blockIdx.x * 256 + threadIdx.x's
// being its own (nullptr: the column holds the whole stack). No cull: a kernel that has one sets it afterwards, as does one that numbers its lanes otherwise.
TD Tracer unstaged_tracer ( const DevScene& sc, int* words, uint32_t stack_depth, uint32_t leaf_cap, uint32_t* spill, uint32_t spill_cap ) {
    Tracer T;
    T.sc = sc; T.l_nodes = nullptr; T.l_tris = nullptr; T.l_props = nullptr; T.l_ranked = nullptr; T.n_boxes = 0;
    T.l_mats = sc.mats; T.l_lights = sc.lights; T.l_area = sc.tri_area;
    T.lds_nodes = 0; T.lds_tris = 0; T.ranked = false; T.pairs = false;
    T.stack = words + threadIdx.x; T.leaves = words + stack_depth * TERRA_COL + threadIdx.x; T.leaf_cap = ( int ) leaf_cap; T.stack_cap = ( int ) stack_depth;
    T.stack_lim = ( uint32_t ) ( uintptr_t ) words + stack_depth * 1024u;
    T.spill = spill ? spill + ( size_t ) ( blockIdx.x * 256u + threadIdx.x ) * spill_cap : nullptr; T.spill_cap = spill ? spill_cap : 0u;
    T.faults = nullptr; T.cull = false; T.fused = false;
    return T;
}

// -----------------------------------------------------------------------------
// BVH traversal (reference src/TerraBVH.c:250-310), restructured without changing
// what is computed:
//   * the node loop only does slab tests and stack traffic; leaves met on the way are
//     appended to a per-lane list and tested afterwards in the order they were met.
//     The reference never lets a hit influence the traversal (no culling against the
//     closest hit), so testing the leaves later, in the same order, with the same
//     strict "<" on depth, selects the same triangle;
//   * when a lane's list is full the lists are drained and the node loop resumes;
//   * the hit point is formed once, from the winning depth (same expression).
// MODE 0: nodes/triangles from global memory; 1: everything staged in LDS.
// -----------------------------------------------------------------------------
struct Closest { float depth; uint32_t tri; };

// Stack / leaf-list writes. A TERRA_CHECK_BOUNDS build (python -m terra_amd.build --variant chk -DTERRA_CHECK_BOUNDS=1)
// refuses (drops the entry, so the column is never left) and counts any write beyond the sizes the host planned; the shipped build trusts the plan
// (max_stack is the exact worst case of the tree, computed at commit).
#ifndef TERRA_CHECK_BOUNDS
#define TERRA_CHECK_BOUNDS 0
#endif
#define TERRA_PUSH(T, sp, v) do { if ( TERRA_CHECK_BOUNDS && ( sp ) >= ( T ).stack + ( T ).stack_cap * TERRA_COL ) { if ( ( T ).faults ) atomicAdd ( ( T ).faults, 1ull ); } else { *( sp ) = ( int ) ( v ); ( sp ) += TERRA_COL; } } while ( 0 )
#define TERRA_LEAF(T, lp, v) do { if ( TERRA_CHECK_BOUNDS && ( lp ) >= ( T ).leaves + ( T ).leaf_cap * TERRA_COL ) { if ( ( T ).faults ) atomicAdd ( ( T ).faults, 1ull ); } else { *( lp ) = ( int ) ( v ); ( lp ) += TERRA_COL; } } while ( 0 )

// which copy of each axis a lane reads from a staged node (byte offsets inside the node); regular rays only. oi = origin * inverse direction, for the
// fused form of the slab test (slab_near_far_fused)
struct SlabSel { uint32_t x, y, z; V3 oi; };
TD SlabSel slab_sel ( const Ray& r ) {
    SlabSel s;
    s.x = r.inv.x < 0.f ? 16u : 0u; s.y = r.inv.y < 0.f ? 48u : 32u; s.z = r.inv.z < 0.f ? 80u : 64u;
    s.oi = v3 ( r.o.x * r.inv.x, r.o.y * r.inv.y, r.o.z * r.inv.z );
    return s;
}

// one node of the reference traversal (src/TerraBVH.c:262-303): pop, slab-test both child boxes, push the inner children
// that are hit, append the leaf children to the lane's list (all of them; with Tracer::cull only those whose box is hit).
// An empty child slot (scenes with < 2 triangles) travels as a leaf and is dropped by leaf_step.
// RANKED (MODE 1, ranked launches): the leaf children go into the lane's rank set `leaf_set` (their bits in the staged node) instead of the list; `lp` is not used.
template <int COUNT, int MODE, bool FAST, bool FUSED = false, bool RANKED = false>
TD void node_step ( const Tracer& T, const Ray& r, const SlabSel& sel, int*& sp, int*& lp, uint32_t& leaf_set, Counters& c ) {
    PS_WAVE ( c, kPsNodeIter ); PS_LANE ( c, kPsNodeLanes );
    sp -= TERRA_COL;
    const uint32_t w = ( uint32_t ) * sp;
    uint32_t child0, child1, bit0 = 0u, bit1 = 0u; bool hit0, hit1;
    float te0 = 0.f, te1 = 0.f;          // (FUSED) entry distance of each child box (unused: kept out of registers by the optimiser)
    if ( MODE == 1 ) {
        const char* node = reinterpret_cast<const char*> ( T.l_nodes ) + w;          // w = byte offset of the staged node
        if ( RANKED ) {
            const uint4 cw = *reinterpret_cast<const uint4*> ( node + 96 );
            child0 = cw.x; child1 = cw.y; bit0 = cw.z; bit1 = cw.w;
        } else {
            const uint2 cw = *reinterpret_cast<const uint2*> ( node + 96 );
            child0 = cw.x; child1 = cw.y;
        }
        if ( FAST ) {
            const float4 ax = *reinterpret_cast<const float4*> ( node + sel.x ), ay = *reinterpret_cast<const float4*> ( node + sel.y ), az = *reinterpret_cast<const float4*> ( node + sel.z );
            if ( FUSED ) {
                hit0 = slab_near_far_fused ( ax.x, ax.y, ay.x, ay.y, az.x, az.y, r, sel.oi, te0 );
                hit1 = slab_near_far_fused ( ax.z, ax.w, ay.z, ay.w, az.z, az.w, r, sel.oi, te1 );
            } else {
                hit0 = slab_near_far ( ax.x, ax.y, ay.x, ay.y, az.x, az.y, r );
                hit1 = slab_near_far ( ax.z, ax.w, ay.z, ay.w, az.z, az.w, r );
            }
        } else {
            const float4 ax = *reinterpret_cast<const float4*> ( node ), ay = *reinterpret_cast<const float4*> ( node + 32 ), az = *reinterpret_cast<const float4*> ( node + 64 );
            hit0 = slab<false> ( v3 ( ax.x, ay.x, az.x ), v3 ( ax.y, ay.y, az.y ), r );
            hit1 = slab<false> ( v3 ( ax.z, ay.z, az.z ), v3 ( ax.w, ay.w, az.w ), r );
        }
    } else {
        const float4* g_nodes = reinterpret_cast<const float4*> ( T.sc.nodes );
#if TERRA_PHASE_STATS
        c.ps[kPsTop64] += w < 64u; c.ps[kPsTop256] += w < 256u; c.ps[kPsTop1024] += w < 1024u; c.ps[kPsTop4096] += w < 4096u;
#endif
        const float4 q0 = g_nodes[4 * w], q1 = g_nodes[4 * w + 1], q2 = g_nodes[4 * w + 2], q3 = g_nodes[4 * w + 3];
        child0 = __float_as_uint ( q3.x ); child1 = __float_as_uint ( q3.y );
        hit0 = slab<FAST> ( v3 ( q0.x, q0.y, q0.z ), v3 ( q0.w, q1.x, q1.y ), r );
        hit1 = slab<FAST> ( v3 ( q1.z, q1.w, q2.x ), v3 ( q2.y, q2.z, q2.w ), r );
    }
    if ( COUNT ) ++c.nodes;
    const bool leaf0 = ( child0 & DEV_CHILD_LEAF ) != 0, leaf1 = ( child1 & DEV_CHILD_LEAF ) != 0;
    if ( !leaf0 && hit0 ) { TERRA_PUSH ( T, sp, child0 ); }
    if ( !leaf1 && hit1 ) { TERRA_PUSH ( T, sp, child1 ); }
    if ( RANKED ) {          // (bit = 0 for an inner child and for an empty slot: nothing to test, as leaf_step drops the empty slot)
        leaf_set |= ( hit0 || !T.cull ) ? bit0 : 0u;
        leaf_set |= ( hit1 || !T.cull ) ? bit1 : 0u;
    } else {
        if ( leaf0 && ( hit0 || !T.cull ) ) { TERRA_LEAF ( T, lp, ( child0 & 0x7fffffffu ) ); }
        if ( leaf1 && ( hit1 || !T.cull ) ) { TERRA_LEAF ( T, lp, ( child1 & 0x7fffffffu ) ); }
    }
    if ( COUNT == 2 && T.cull ) c.tri_culled += ( uint32_t ) ( leaf0 && !hit0 ) + ( uint32_t ) ( leaf1 && !hit1 );
}

// triangle test of one entry of the lane's leaf list, in the order the leaves were met: strict "<" keeps the first of equal depths
// (expected != none: the ray only asks whether its closest hit is triangle `expected` -- scene_raycast_triangle -- and `stop` is set by the first other triangle that comes first)
template <int COUNT, int MODE, bool ANYHIT = false>
TD void leaf_step ( const Tracer& T, const int* entry, const RayState& st, V3 o_perm, Closest& best, Counters& c, uint32_t expected = 0xffffffffu, bool* stop = nullptr ) {
    const float4* g_tris = reinterpret_cast<const float4*> ( T.sc.tris );
    PS_WAVE ( c, kPsLeafIter ); PS_LANE ( c, kPsLeafLanes );
    const uint32_t ti = ( uint32_t ) * entry;
    if ( ti == ( DEV_CHILD_EMPTY & 0x7fffffffu ) ) return;           // the empty slot of a degenerate tree
    const TriPerm tp = MODE == 1 ? tri_perm_lds ( T.l_tris + 12 * ti, st ) : tri_perm ( g_tris[3 * ti], g_tris[3 * ti + 1], g_tris[3 * ti + 2], st );
    if ( COUNT ) ++c.tri_tests;
    float depth;
    if ( watertight_permuted ( tp, o_perm, st, depth ) && depth < best.depth ) { best.depth = depth; best.tri = ti; if ( ANYHIT && ti != expected ) *stop = true; }
}

// Ranked launches (MODE 1, Tracer::ranked). The leaves any ray meets are a subsequence of one global order -- the order in which the traversal with every box
// hit meets them (scene_host.cpp leaf_ranks) --, so "test the listed leaves in the order met" is "test the set ranks from low to high": the same triangles,
// in the same order, with the same strict "<". The node loop therefore runs to the end in one pass and only sets bits; the leaf loop then walks the set
// bits and reads each triangle, already permuted into the ray's axes, with three 16-byte loads from the copy for the ray's permutation.
// The flat form of a ranked launch's node loop (see "Flat leaf-box test" above): every lane tests every staged box, with the floats and the arithmetic node_step
// applies to that box on a FUSED walk, and collects the masks of the boxes it passes. The set can only exceed the walk's by leaves whose own box passes while an
// ancestor's fails; by the containment property the commit verifies (a triangle the ray hits lies inside every box built around it as the box
// test sees it) such a triangle is not hit, so the closest hit, the tie-breaks and the ANYHIT answers are the walk's.
// (TERRA_PHASE_STATS builds count one node iteration per box tested.)
// Addresses. A lane's three plane pairs of box k lie at bx / by / bz + TERRA_LEAF_BOX_STRIDE * k, where b<axis> = the 32-bit LDS address of the table's slot
// (axis, sign of the ray's direction there) in box 0: terra_leaf_box_plane_offset ( 0, a, s ), formed once per traversal in table units (a select between two
// constants per axis: no SlabSel offset is scaled). The whole table is within reach of a ds_read's 16-bit immediate from there (TERRA_LEAF_BOX_REACH), so a
// trip's reads are immediates on one moving base per axis. The bases go through an empty asm statement: it hides from the optimiser that they are "start of the
// dynamic LDS segment + offset", which it otherwise keeps apart to re-add the segment's start (the constant 0) in front of every read. The masks are wave-uniform:
// their address is scalar arithmetic, one move into the address register per trip.
// The 32-bit LDS address of a staged word is the low half of its generic pointer (the shared aperture's base has no low bits; the compiler's own cast to
// address space 3 takes the same half, and Tracer::stack_lim is formed the same way). The empty asm statements serve speed only: without them the code is as right
// and a few instructions longer, and nothing fails -- after a compiler upgrade read the trip counts again (python tools/isa_cost.py --loops: 96 / 50 / 16; the pair
// form with its four key instructions per box: 128 / 66 / 21). The one asm statement that is not empty, leaf_box_test's v_bfi_b32, computes: it IS (te & ~31) | entry.
typedef float PlanePair __attribute__ (( ext_vector_type ( 2 ) ));          // (a built-in vector: the host pass, too, can read one through an LDS pointer)
typedef const __attribute__ (( address_space ( 3 ) )) PlanePair* LdsPlanes;
// Nearest first (PAIRS only; "Nearest first" below): lo / hi = the smallest and second-smallest key among the boxes the lane passes, key = the bits of the box's entry
// distance with the low five replaced by the box's number `entry` (wave-uniform: the scalar operand of one v_bfi_b32; below 32), TERRA_NO_BOX for a box it misses.
// Compared as SIGNED words: an entry distance is >= +0 or is -0, and -0 then sorts first and fails the cut as a float bound -- the safe side both times.
#define TERRA_NO_BOX 0x7fffffff
struct NearestBoxes { int32_t lo, hi; };
template <bool PAIRS>
TD void leaf_box_test ( uint32_t bx, uint32_t by, uint32_t bz, const char* pm, const Ray& r, const SlabSel& sel, uint32_t& leaf_set, Counters& c, uint32_t entry, NearestBoxes& nb ) {
    PS_WAVE ( c, kPsNodeIter ); PS_LANE ( c, kPsNodeLanes );
    const PlanePair ax = * ( LdsPlanes ) ( uintptr_t ) bx, ay = * ( LdsPlanes ) ( uintptr_t ) by, az = * ( LdsPlanes ) ( uintptr_t ) bz;
    const uint32_t m = *reinterpret_cast<const uint32_t*> ( pm );          // (read whether or not the box is hit: a select, not a branch around a load)
    float te;
    const bool hit = slab_near_far_fused ( ax.x, ax.y, ay.x, ay.y, az.x, az.y, r, sel.oi, te );
    leaf_set |= hit ? m : 0u;
    if constexpr ( PAIRS ) {
        // (te & ~31) | entry as one instruction: a bit-field insert under the inline constant 31 with the entry as its one scalar operand. Written out, the compiler
        // takes a v_and_b32 with the literal ~31 and a v_or3_b32 -- or, asked for the insert in C, holds ~31 in a scalar and moves every entry to a vector register.
        uint32_t bits;
        asm ( "v_bfi_b32 %0, 31, %1, %2" : "=v" ( bits ) : "s" ( entry ), "v" ( te ) );
        const int32_t key = hit ? ( int32_t ) bits : TERRA_NO_BOX;
        const int32_t lo = nb.lo, hi = nb.hi;
        nb.lo = key < lo ? key : lo;
        nb.hi = __builtin_elementwise_max ( __builtin_elementwise_min ( lo, hi ), __builtin_elementwise_min ( __builtin_elementwise_max ( lo, hi ), key ) );      // (v_med3_i32: with lo <= hi the median is the second smallest of the three)
    }
}
// N boxes at immediate offsets from the bases, which then move on to the next box. STRIDE: from a box's plane pairs to the next one's, in the form in use
template <int N, uint32_t STRIDE, bool PAIRS>
TD void leaf_box_group ( uint32_t& bx, uint32_t& by, uint32_t& bz, const char*& pm, const Ray& r, const SlabSel& sel, uint32_t& leaf_set, Counters& c, uint32_t& entry, NearestBoxes& nb ) {
    #pragma unroll
    for ( int k = 0; k < N; ++k )
        leaf_box_test<PAIRS> ( bx + STRIDE * k, by + STRIDE * k, bz + STRIDE * k, pm + TERRA_LEAF_BOX_MASK_STRIDE * k, r, sel, leaf_set, c, entry + ( uint32_t ) k, nb );
    bx += STRIDE * N; by += STRIDE * N; bz += STRIDE * N; pm += TERRA_LEAF_BOX_MASK_STRIDE * N;
    if constexpr ( PAIRS ) entry += ( uint32_t ) N;
}
// PAIRS: the table lies in the pair section's own part (dev_types.h "pair form") and its masks are in entry bits; otherwise in the pad words of the ranked entries
template <bool PAIRS>
TD uint32_t leaf_boxes_flat ( const Tracer& T, const Ray& r, const SlabSel& sel, Counters& c, NearestBoxes& nb ) {
    constexpr uint32_t kStride = PAIRS ? ( uint32_t ) TERRA_PAIR_BOX_STRIDE : ( uint32_t ) TERRA_LEAF_BOX_STRIDE;
    constexpr uint32_t kX = PAIRS ? terra_pair_box_plane_offset ( 0, 0, 0 ) : terra_leaf_box_plane_offset ( 0, 0, 0 ), kY = PAIRS ? terra_pair_box_plane_offset ( 0, 1, 0 ) : terra_leaf_box_plane_offset ( 0, 1, 0 ),
                       kZ = PAIRS ? terra_pair_box_plane_offset ( 0, 2, 0 ) : terra_leaf_box_plane_offset ( 0, 2, 0 );
    const uint32_t table = ( uint32_t ) ( uintptr_t ) T.l_ranked + ( PAIRS ? terra_pair_boxes_offset ( T.lds_tris >> 1 ) : 0u );
    constexpr uint32_t kNeg = PAIRS ? terra_pair_box_plane_offset ( 0, 0, 1 ) - terra_pair_box_plane_offset ( 0, 0, 0 ) : terra_leaf_box_plane_offset ( 0, 0, 1 ) - terra_leaf_box_plane_offset ( 0, 0, 0 );      // from an axis' (near, far) for a positive direction to the one for a negative
    uint32_t sx = r.inv.x < 0.f ? kNeg : 0u, sy = r.inv.y < 0.f ? kNeg : 0u, sz = r.inv.z < 0.f ? kNeg : 0u;      // (the signs slab_sel goes by)
    asm ( "" : "+v" ( sx ), "+v" ( sy ), "+v" ( sz ) );          // (kept a select between two inline constants and one add of a wave-uniform base each)
    uint32_t bx = table + kX + sx, by = table + kY + sy, bz = table + kZ + sz;
    asm ( "" : "+v" ( bx ), "+v" ( by ), "+v" ( bz ) );
    const char* pm = reinterpret_cast<const char*> ( T.l_props ) + terra_leaf_box_mask_offset ( 0 );
    uint32_t leaf_set = 0u, entry = 0u;
    if constexpr ( PAIRS ) nb.lo = nb.hi = TERRA_NO_BOX;
    // one group at a time, as written. Cross-compiled for gfx950 without these pragmas (profiles/leaf_boxes/kernel_resources.md): left to unroll, the loads of
    // several groups are hoisted together and the Simple kernel takes 1,728 B of scratch; vectorised two groups wide, the tests become v_pk_fma_f32 fed by moves
    // (104 B of scratch; build.py on why the build keeps packed arithmetic out). With them: no scratch
    #pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for ( uint32_t g = T.n_boxes / TERRA_LEAF_BOX_GROUP; g != 0; --g ) leaf_box_group<TERRA_LEAF_BOX_GROUP, kStride, PAIRS> ( bx, by, bz, pm, r, sel, leaf_set, c, entry, nb );
    if ( T.n_boxes & 4u ) leaf_box_group<4, kStride, PAIRS> ( bx, by, bz, pm, r, sel, leaf_set, c, entry, nb );
    #pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for ( uint32_t k = T.n_boxes % 4u; k != 0; --k ) leaf_box_group<1, kStride, PAIRS> ( bx, by, bz, pm, r, sel, leaf_set, c, entry, nb );
    return leaf_set;
}

// The pair form of a ranked traversal (see "Pair form" above). The node part is the ranked one -- the flat loop over the pair section's table, or the walk, whose
// staged nodes carry entry bits --; the leaf loop walks the set entries, one pair per trip.
// Record rule. Entry order is not rank order across pairs (the Cornell box has pairs of ranks (2, 4) and (3, 12)), so "first met wins a tie" cannot be left to the
// order of the trips: the record is the lexicographic minimum of (depth, key), key = terra_pair_key ( rank, triangle ), which is what the reference's order with its
// strict "<" selects -- among equal depths the triangle met first, i.e. of the lowest rank. The record starts as (FLT_MAX, 0): no key is below 0, so a hit at FLT_MAX
// is refused as the strict "<" refuses it. ANYHIT: the record is preset to the expected triangle's own (depth, key) (scene_raycast_triangle); the first triangle
// that beats it comes first in the reference's order too, and ends the loop with key 0 ("another one"); the expected triangle itself never beats its own record.
// Nearest first (Tracer::nearest; flat launches of a table in which box k holds exactly entry k). The reference never culls against the closest hit, so a lane's set
// is every quad on the ray's line and the wave's trip count is its longest such line, although only the nearest quad can win. The flat loop therefore keeps the two
// smallest entry distances of the boxes a lane passes (leaf_box_test), and the leaf loop
//   * tests the entry of the nearest box first (lo & 31), then the lowest entry left, as before;
//   * after every trip drops the whole set once depth_best < cut, cut = the second-smallest key with its index bits cleared: an entry distance rounded DOWN.
// Why no bit can move. The record rule does not depend on the order of the trips, so only the dropped entries matter. Every entry j still in the set after the first
// trip has t_enter_j >= cut (cut is a lower bound of the second smallest, and the smallest has been tested). A triangle of entry j that the ray hits lies inside its
// own extent, i.e. at least 1e-4 inside its box (the extent grown by 1e-4) on every axis, so the ray's true entry parameter into the box is below the true depth by at
// least 1e-4 / |d|. The computed t_enter carries the two roundings of the fused slab form, the computed depth the watertight test's error; both are inside the
// < 56 u R / |d| the commit's containment check budgets (scene_host.cpp "numeric containment check": admitted only where 128 u R <= 1e-4, and the flat form runs only
// there, on tame rays). Hence computed t_enter_j < computed depth_j, and with depth_best < cut <= t_enter_j < depth_j the triangle is strictly beyond the record: it
// wins neither by depth nor, among equal depths, by key. Nothing is assumed of |d| -- ray-sourced launches do not normalise --: t_enter and depth are parameters along
// the same d and scale alike, as do their error bounds. tests/test_leaf_nearest.py holds the inequality on the host with the device's operations.
// Where the cut fails -- the first trip misses its pair and the record stays FLT_MAX, a tie keeps cut from lying strictly beyond the record, cut is -0 or the NaN of
// "no second box" -- every entry left is tested in bit order as before: exact whatever the first trip did.
// ANYHIT: a preset record strictly below the smallest entry distance cannot be beaten and the loop is skipped; otherwise the nearest entry goes first, the first
// triangle that beats the record ends the loop as before, and the cut applies with the preset record.
template <int COUNT, int MODE, bool FAST, bool FUSED, bool ANYHIT, class RS = RayState>
TD void traverse_pairs ( const Tracer& T, const Ray& r, const RS& st, V3 o_perm, Closest& best, Counters& c ) {
    const SlabSel sel = slab_sel ( r );
    uint32_t leaf_set = 0u;
    PS_WAVE ( c, kPsDrainIter );
    bool flat = false;
    if constexpr ( FUSED ) flat = T.n_boxes != 0u;
    NearestBoxes nb; nb.lo = nb.hi = TERRA_NO_BOX;
    bool nearest = false;
    if ( flat ) { leaf_set = leaf_boxes_flat<true> ( T, r, sel, c, nb ); nearest = T.nearest; }          // (launch constant)
    else {
        int* sp = T.stack; int* lp = nullptr;
        *sp = 0; sp += TERRA_COL;
        while ( sp != T.stack ) node_step<COUNT, MODE, FAST, FUSED, true> ( T, r, sel, sp, lp, leaf_set, c );
    }
    const uint32_t perm = ray_perm ( st );
    const float4* copy = T.l_ranked + ( TERRA_PAIR_ENTRY_BYTES / 16 ) * ( T.lds_tris >> 1 ) * perm;
    float depth_best = best.depth; uint32_t key_best = ANYHIT ? best.tri : 0u;          // (ANYHIT: the caller's preset key travels in best.tri; the record itself never moves)
    bool beaten = false;
    // Nearest first: the first trip tests the entry of the nearest box the lane passes, every later one the lowest entry left; after each trip the set is dropped
    // once the record lies strictly below `cut`, the second-smallest entry distance rounded down -- a lower bound of the entry distance of every entry still in the
    // set, and an entry's triangles lie beyond their box's entry distance. Without it (the walk, the switch off) cut is a NaN: no record is below it.
    const float cut = __uint_as_float ( ( uint32_t ) ( nearest ? nb.hi : TERRA_NO_BOX ) & ~31u );
    if ( ANYHIT && nearest && depth_best < __uint_as_float ( ( uint32_t ) nb.lo & ~31u ) ) leaf_set = 0u;          // the preset record lies in front of every box passed
    uint32_t next = nearest ? ( uint32_t ) nb.lo & 31u : ( uint32_t ) __builtin_ctz ( leaf_set | 0x80000000u );          // (an empty set: never used)
    while ( leaf_set != 0u ) {
        PS_WAVE ( c, kPsLeafIter ); PS_LANE ( c, kPsLeafLanes );
        const float4* e = copy + ( TERRA_PAIR_ENTRY_BYTES / 16 ) * next;
        leaf_set &= ~ ( 1u << next );
        const uint2 keys = *reinterpret_cast<const uint2*> ( e + 3 );
        auto load = [&] ( bool again ) {
            uint32_t a = ( uint32_t ) ( uintptr_t ) e;
            if ( again ) asm volatile ( "" : "+v" ( a ) );          // (the second read is a read: see watertight_pair)
            typedef float Piece __attribute__ (( ext_vector_type ( 4 ) ));          // (a built-in vector, as PlanePair)
            const __attribute__ (( address_space ( 3 ) )) Piece* q = ( const __attribute__ (( address_space ( 3 ) )) Piece* ) ( uintptr_t ) a;
            const Piece q0 = q[0], q1 = q[1], q2 = q[2];
            return PairPerm { { q0.x, q0.y, q0.z }, { q0.w, q1.x, q1.y }, { q1.z, q1.w, q2.x }, { q2.y, q2.z, q2.w } };
        };
        watertight_pair ( load, o_perm, st, [&] ( float depth, bool second ) {
            const uint32_t key = second ? keys.y : keys.x;
            if ( ( depth < depth_best ) | ( ( depth == depth_best ) & ( key < key_best ) ) ) {
                if ( ANYHIT ) { beaten = true; leaf_set = 0u; }
                else { depth_best = depth; key_best = key; }
            }
        } );
        if ( depth_best < cut ) leaf_set = 0u;
        next = ( uint32_t ) __builtin_ctz ( leaf_set | 0x80000000u );
    }
    best.depth = depth_best;
    best.tri = ANYHIT ? ( beaten ? 0u : key_best ) : ( key_best ? ( key_best & 31u ) : 0xffffffffu );
}

template <int COUNT, int MODE, bool FAST, bool FUSED = false, bool ANYHIT = false, class RS = RayState>
TD void traverse_ranked ( const Tracer& T, const Ray& r, const RS& st, V3 o_perm, Closest& best, Counters& c, uint32_t expected ) {
    if constexpr ( COUNT == 0 ) if ( T.pairs ) { traverse_pairs<COUNT, MODE, FAST, FUSED, ANYHIT> ( T, r, st, o_perm, best, c ); return; }      // (launch constant)
    const SlabSel sel = slab_sel ( r );
    uint32_t leaf_set = 0u;
    PS_WAVE ( c, kPsDrainIter );
    bool flat = false;
    if constexpr ( COUNT == 0 && FUSED ) flat = T.n_boxes != 0u;     // (launch constant; FUSED: the wave's rays are all tame)
    NearestBoxes no_nb;          // (single form: never written)
    if ( flat ) leaf_set = leaf_boxes_flat<false> ( T, r, sel, c, no_nb );
    else {
        int* sp = T.stack; int* lp = nullptr;
        *sp = 0; sp += TERRA_COL;                                      // the root: node 0 = byte offset 0
        while ( sp != T.stack ) node_step<COUNT, MODE, FAST, FUSED, true> ( T, r, sel, sp, lp, leaf_set, c );
    }
    const uint32_t perm = ray_perm ( st );
    const float4* copy = T.l_ranked + 3u * T.lds_tris * perm;
    while ( leaf_set != 0u ) {
        PS_WAVE ( c, kPsLeafIter ); PS_LANE ( c, kPsLeafLanes );
        const float4* e = copy + 3u * ( uint32_t ) __builtin_ctz ( leaf_set );
        leaf_set &= leaf_set - 1u;
        const float4 q0 = e[0], q1 = e[1], q2 = e[2];
        const TriPerm tp = { { q0.x, q0.y, q0.z }, { q0.w, q1.x, q1.y }, { q1.z, q1.w, q2.x } };
        if ( COUNT ) ++c.tri_tests;
        float depth;
        if ( watertight_permuted ( tp, o_perm, st, depth ) && depth < best.depth ) {
            const uint32_t ti = __float_as_uint ( q2.y );
            best.depth = depth; best.tri = ti;
            if ( ANYHIT && ti != expected ) leaf_set = 0u;             // another triangle comes first: nothing further can change the answer
        }
    }
}

template <int COUNT, int MODE, bool FAST, bool FUSED = false, bool ANYHIT = false, class RS = RayState>
TD void traverse_loops ( const Tracer& T, const Ray& r, const RS& st, V3 o_perm, Closest& best, Counters& c, uint32_t expected = 0xffffffffu ) {
    if constexpr ( MODE == 1 ) if ( T.ranked ) { traverse_ranked<COUNT, MODE, FAST, FUSED, ANYHIT> ( T, r, st, o_perm, best, c, expected ); return; }
    const SlabSel sel = slab_sel ( r );
    int* sp = T.stack; int* lp = T.leaves;
    int* const lp_full = T.leaves + ( T.leaf_cap - 2 ) * TERRA_COL;       // a node adds at most two leaves
    uint32_t no_set = 0u;
    *sp = 0; sp += TERRA_COL;                                          // the root: node 0 = byte offset 0
    for ( ;; ) {
        PS_WAVE ( c, kPsDrainIter );
        while ( sp != T.stack && lp <= lp_full ) node_step<COUNT, MODE, FAST, FUSED> ( T, r, sel, sp, lp, no_set, c );
        if constexpr ( ANYHIT ) {
            bool stop = false;
            for ( const int* e = T.leaves; e != lp && !stop; e += TERRA_COL ) leaf_step<COUNT, MODE, true> ( T, e, st, o_perm, best, c, expected, &stop );
            if ( stop ) sp = T.stack;                                  // another triangle comes first: nothing further can change the answer
        } else
        for ( const int* e = T.leaves; e != lp; e += TERRA_COL ) leaf_step<COUNT, MODE> ( T, e, st, o_perm, best, c );
        lp = T.leaves;
        if ( sp == T.stack ) break;
    }
}

// the same from a ray start that brings the origin in the ray's axes along (trace_geometry.h ray_start_masks) and what make_ray_guarded found in the wave:
// all_guarded answers both votes (trace_geometry.h "One range test per ray"). (bvh_traverse above keeps its own text: written as a call of this one with
// all_guarded = false it compiles to the same instructions in another order, and every kernel but seven is held to the code it had.)
template <int COUNT, int MODE, class RS>
TD Closest bvh_traverse_from ( const Tracer& T, const Ray& r, const RS& st, V3 o_perm, Counters& c, bool all_guarded ) {
    Closest best; best.depth = FLT_MAX; best.tri = 0xffffffffu;
    // the slab variant is chosen per WAVE: one irregular ray sends its whole wave down the exact path
    const bool guarded = all_guarded;
    if ( MODE == 1 && T.fused && ( guarded || __all ( ray_is_tame ( r ) ) ) ) traverse_loops<COUNT, MODE, true, true> ( T, r, st, o_perm, best, c );
    else if ( guarded || __all ( ray_is_regular ( r ) ) ) traverse_loops<COUNT, MODE, true> ( T, r, st, o_perm, best, c );
    else traverse_loops<COUNT, MODE, false> ( T, r, st, o_perm, best, c );
    return best;
}
template <int COUNT, int MODE>
TD Closest bvh_traverse ( const Tracer& T, const Ray& r, const RayState& st, Counters& c ) {
    Closest best; best.depth = FLT_MAX; best.tri = 0xffffffffu;
    V3 o_perm = permuted ( r.o, st );
    // the slab variant is chosen per WAVE: one irregular ray sends its whole wave down the exact path
    if ( MODE == 1 && T.fused && __all ( ray_is_tame ( r ) ) ) traverse_loops<COUNT, MODE, true, true> ( T, r, st, o_perm, best, c );
    else if ( __all ( ray_is_regular ( r ) ) ) traverse_loops<COUNT, MODE, true> ( T, r, st, o_perm, best, c );
    else traverse_loops<COUNT, MODE, false> ( T, r, st, o_perm, best, c );
    return best;
}

// -----------------------------------------------------------------------------
// Resumable traversal for the decoupled render loop (large scenes; render_kernels.hip).
// The 64 lanes of a wave hold DIFFERENT rays at different stages; a lane's traversal state
// (stack column and leaf list in LDS; top, nleaf, closest hit in registers) survives leaving
// and re-entering these functions. They return as soon as the number of lanes that still
// have nodes to visit has dropped to `exit_active`, so that the finished lanes can be shaded
// and given their next ray instead of idling until the slowest ray of the wave is done
// (on the 97k-triangle hall a ray visits 474 nodes on average with a long tail: waiting for
// the slowest of 64 left 17 % of the lanes busy). What is computed per ray, and in which
// order, is exactly what traverse_loops computes.
// `traversing` is cleared for lanes whose traversal completed.
// -----------------------------------------------------------------------------
template <int COUNT, int MODE, bool FAST>
TD void traverse_resume ( const Tracer& T, const Ray& r, const SlabSel& sel, const RayState& st, V3 o_perm, Closest& best, int*& sp, bool& traversing, int exit_active, Counters& c ) {
    int* const lp_full = T.leaves + ( T.leaf_cap - 2 ) * TERRA_COL;
    int* lp = T.leaves;                                      // every lane's list is empty on entry and on exit
    uint32_t no_set = 0u;
    for ( ;; ) {
        for ( ;; ) {
            const bool can = traversing && sp != T.stack && lp <= lp_full;
            const int n_can = __popcll ( __ballot ( can ) ), n_nodes = __popcll ( __ballot ( traversing && sp != T.stack ) );
            if ( n_can == 0 || n_nodes <= exit_active ) break;
            if ( can ) node_step<COUNT, MODE, FAST> ( T, r, sel, sp, lp, no_set, c );
        }
        for ( const int* e = T.leaves; e != lp; e += TERRA_COL ) leaf_step<COUNT, MODE> ( T, e, st, o_perm, best, c );        // lanes that are not traversing hold an empty list
        lp = T.leaves;
        if ( traversing && sp == T.stack ) traversing = false;
        if ( __popcll ( __ballot ( traversing ) ) <= exit_active ) break;
    }
}
