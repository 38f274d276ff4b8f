// traverse_fast.h -- traversal of the optional fast tree, template MODE 2 / 3 (trace_device.h lists the layers).
#pragma once
#include "traverse_ref.h"

// -----------------------------------------------------------------------------
// MODE 2: traversal of the optional fast tree (DESIGN.md "Fast tree"). Not the reference's
// traversal: near child first, subtrees whose entry distance exceeds the closest hit are
// culled, leaves hold up to 4 triangles. It returns the reference's answer because the
// reference's closest hit is order independent once ties are resolved the way its fixed
// leaf visit order resolves them: smallest depth, then smallest reference visit rank
// (DevTri::pad of the fast soup). The triangle test itself is the same arithmetic.
// Child word of a fast node: bit 31 leaf; leaf = (count-1) << 27 | first triangle.
//
// Node format in HBM (DevFastNode, 128 B = one cache line, FOUR children; made on the host by tree_build.cpp fastbvh::widen): the planes of the child boxes as binary16,
// rounded OUTWARD, one 32-bit word per child and axis, the four children's words of one axis side by side -- and each such 16-byte group TWICE: as (min | max << 16)
// for rays that travel in the axis' positive direction and as (max | min << 16) for the others --, then the four child words. A ray loads, per axis, the group whose
// low half is ITS near plane (three offsets it computes once), plus the child words: four 16-byte loads fetch what it needs of a node, 64 of the 128 bytes.
// What binds the render kernels of scenes read from global memory (profiles/r04_measurements/ab_fast_node_formats.log): (1) the texture addresser -- ~21-27 of its
// cycles per wave-level load instruction whatever the instruction's width, 99 % busy when a node step issues 4 loads for 2 boxes -- so what counts is the NUMBER of
// load instructions per ray, not their bytes; (2) the dependent chain: a ray's node fetches follow one another, and the waves spend 54 % of their cycles waiting;
// (3) VALU issue. A 4-wide node of binary16 planes answers (1) and (2): 4 loads bring 4 boxes (the 64-byte (min, max) node of rounds 2-3 brought 2), and a ray needs
// half as many round trips. Each plane goes straight into t = fma ( plane, inv, -(o * inv) ) as the binary16 operand of v_fma_mix_f32 (op_sel picks the half): a box
// costs six fused multiply-adds, a v_max3, a v_min3 and the comparisons. (Until round 4's third session a node was 64 bytes with one (min | max << 16) word per child
// and axis, and the ray swapped the halves with a v_perm_b32 per box and axis: twelve more VALU instructions per node step on a kernel bound by VALU issue; choosing
// the group by ADDRESS costs three adds. Hall 198.9 -> 193.3 ms, sphere scene 302.2 -> 293.8: profiles/r04_measurements/ab_fast_tree_builder.log.) Unlike the
// reference tree's test this one only has to be CONSERVATIVE (never
// reject a box that holds a triangle the ray hits; DESIGN.md "Traversal policy"): rounding the planes outward only widens the box, and t carries two roundings
// (o * inv, the fma) where the commit-time error budget (scene_host.cpp "numeric containment check") allows four. Planes are stored times DevScene::fast_scale (a
// power of two: exact) so that every scene fits binary16's range; the ray's inverse direction is divided by it (exact too).
// An empty child slot is an inverted box (min = +max_half, max = -max_half): never entered, so no lane ever holds it.
// -----------------------------------------------------------------------------
typedef _Float16 terra_half2 __attribute__ (( ext_vector_type ( 2 ) ));
TD terra_half2 as_half2 ( uint32_t u ) { return __builtin_bit_cast ( terra_half2, u ); }
// what a ray needs of itself for the fast tree's box test: the inverse direction -- clamped (a ray parallel to an axis has an infinite inverse direction there, and inf - inf
// would drop that axis from the test: correct but ruinous, such a ray then visits every box along its line; clamped to +-2^100 the axis keeps its meaning: (plane - o) * 2^100
// has the sign of "outside the slab") and divided by the planes' scale --, origin x clamped inverse direction, and per axis the byte offset (inside a node) of the plane group that has the ray's near plane in the low half
struct FastRay { V3 inv, oi; uint32_t px, py, pz; };
TD FastRay fast_ray ( const Ray& ray, float inv_scale ) {
    FastRay f;
    const float cx = __builtin_fminf ( __builtin_fmaxf ( ray.inv.x, -0x1p100f ), 0x1p100f ), cy = __builtin_fminf ( __builtin_fmaxf ( ray.inv.y, -0x1p100f ), 0x1p100f ), cz = __builtin_fminf ( __builtin_fmaxf ( ray.inv.z, -0x1p100f ), 0x1p100f );
    f.oi = v3 ( ray.o.x * cx, ray.o.y * cy, ray.o.z * cz );
    f.inv = v3 ( cx * inv_scale, cy * inv_scale, cz * inv_scale );
    f.px = cx < 0.f ? 16u : 0u; f.py = cy < 0.f ? 48u : 32u; f.pz = cz < 0.f ? 80u : 64u;      // byte offsets of the ray's plane groups inside a node
    return f;
}
// entry distance of one child box from its three plane words (near | far << 16 per axis: the ray loaded the group that has them this way round); hit = the ray's interval inside the box is not empty and starts no later
// than the closest hit so far. `limit_up` = that hit's depth plus one ulp: t_enter <= depth is t_enter < limit_up, which folds into the min3 of the far planes.
TD bool slab_half ( uint32_t wx, uint32_t wy, uint32_t wz, const FastRay& f, float limit_up, float& t_enter ) {
    const terra_half2 x = as_half2 ( wx ), y = as_half2 ( wy ), z = as_half2 ( wz );      // (near, far): the ray loaded the group that has them this way round
    const float tnx = __builtin_fmaf ( ( float ) x.x, f.inv.x, -f.oi.x ), tfx = __builtin_fmaf ( ( float ) x.y, f.inv.x, -f.oi.x );
    const float tny = __builtin_fmaf ( ( float ) y.x, f.inv.y, -f.oi.y ), tfy = __builtin_fmaf ( ( float ) y.y, f.inv.y, -f.oi.y );
    const float tnz = __builtin_fmaf ( ( float ) z.x, f.inv.z, -f.oi.z ), tfz = __builtin_fmaf ( ( float ) z.y, f.inv.z, -f.oi.z );
    t_enter = __builtin_fmaxf ( __builtin_fmaxf ( __builtin_fmaxf ( tnx, tny ), tnz ), 0.f );
    return __builtin_fminf ( __builtin_fminf ( __builtin_fminf ( tfx, tfy ), tfz ), limit_up ) > t_enter;
}

struct ClosestRanked { float depth; uint32_t rank; uint32_t tri; };

// Would the REFERENCE traversal (src/TerraBVH.c:250-310) have tested fast triangle `ti` for this ray? It tests a leaf child whenever it visits the
// leaf's node, and it visits a node when the slab test of that node's box -- stored in its parent -- passed, for every inner node on the way down from
// the root. So: replay that slab test (the reference's compare-select form, unclamped inverse direction) up the parent links. Only scenes outside the
// coordinate range of the containment proof need this (DevScene::reach): inside it, a triangle the ray hits implies all of these tests pass.
#ifndef TERRA_REACH_SELFCHECK      // check builds: replay every level and count (terra_amd_debug_faults) the ones the mask had cleared that fail -- must stay 0
#define TERRA_REACH_SELFCHECK 0
#endif
TD bool reference_reaches ( const Tracer& T, uint32_t ti, const Ray& ray ) {
    const float4* tab = reinterpret_cast<const float4*> ( T.sc.ref_replay );
    // levels whose test can fail at all (DevScene::fast_leaf_mask): the walk ends above the highest of them. The mask's "contains the level below" shortcut
    // needs a regular ray (monotone slab arithmetic, no NaN); any other ray replays every level
    uint32_t mask = ray_is_regular ( ray ) ? T.sc.fast_leaf_mask[ti] : 0xffffffffu;
    uint32_t q = T.sc.fast_leaf_parent[ti];
    bool ok = true;
    while ( q != 0u && ( TERRA_REACH_SELFCHECK || mask != 0u ) ) {
        const float4 a = tab[2 * q], b = tab[2 * q + 1];          // {min, parent} {max, -}
        if ( TERRA_REACH_SELFCHECK || ( mask & 1u ) ) {
            if ( !slab<false> ( v3 ( a.x, a.y, a.z ), v3 ( b.x, b.y, b.z ), ray ) ) {
                if ( !TERRA_REACH_SELFCHECK ) return false;
                // a cleared level that fails while every tested level below it passed: the mask is wrong. (After a tested level has failed, the levels above may
                // fail too -- "contains the level below" only promises that a pass propagates upwards -- and mean nothing.)
                if ( mask & 1u ) ok = false; else if ( ok && T.faults ) atomicAdd ( T.faults, 1ull );
            }
        }
        q = __float_as_uint ( a.w );
        mask = ( mask & 0x80000000u ) | ( mask >> 1 );      // next level (bit 31 stands for every level from 31 up)
    }
    return ok;
}

// A lane's traversal state is its stack and TWO registers. `held`: the leaf whose triangles it is testing (0 = none). `hand`: DEV_CHILD_EMPTY = nothing; a node
// index = the node it descends into next; a leaf word = the next leaf, waiting for `held` to be free. Of the children of a node whose boxes the ray enters, the
// nearest goes into `hand` (so a descent step does not wait for an LDS write + read of its own) -- or straight into `held` when it is a leaf and `held` is free --
// and the others wait on the lane's stack, farthest first. The stack's first entries are an LDS column, the rest -- which a ray almost never reaches: the column
// covers the depths rays actually see, the bound is the tree's worst case -- a few words of HBM per lane (fast_push / fast_pop). A ray starts with the root
// (node 0) in hand and an empty stack.
// Each iteration the wave votes: while fewer than TERRA_FAST_LEAF_16THS / 16 of its busy lanes hold a leaf (and some lane can still descend) the lanes that can
// descend take a node step, otherwise the holders test one triangle each. A lane that holds a leaf does NOT wait for the triangle step: it goes on descending
// towards its next leaf (speculatively: had its held leaf been tested first, the closer hit might have culled some of those nodes) and only stops when that one is
// in hand too. Without this, node steps ran 61 % full and triangle steps 40 % (hall); the few extra node visits cost less than the fuller steps save
// (profiles/r04_measurements/ab_fast_tree_knobs.log). (16/16 would be the classic "while-while" loop: descend until every lane holds a leaf.)
// The traversal is resumable (stack in LDS / HBM; top, hand, held, closest hit in registers): it returns as soon as the number of busy lanes has dropped to
// `exit_active`, so the render loop can shade the finished lanes and hand them their next ray (exit_active = 0: run every lane's ray to the end). A lane is done
// when it holds nothing and its stack is empty (fast_traversing). WHICH nodes a lane visits depends on the votes (on when its held leaf is tested), the closest hit
// it returns does not: that is the minimum over (depth, reference visit rank) of the triangles the ray hits, and no box that holds it is ever culled.
#ifndef TERRA_FAST_LEAF_16THS
#define TERRA_FAST_LEAF_16THS 12
#endif
// (the test "is this entry in the LDS column" compares the entry's 32-bit LDS address with ONE wave-uniform limit: entry e of thread t sits at column base + e * 1024 + t * 4,
//  and t * 4 < 1024, so address < base + cap * 1024 exactly when e < cap; the HBM index is computed on the cold side only)
// (Entries that carry their box's entry distance, so that one the closest hit has overtaken is dropped when it comes off the stack, were measured: 8 % fewer node
//  steps on the hall, 5 % on the sphere scene, and no time gained -- the second word and the pop loop cost what they save. profiles/r04_measurements/ab_fast_tree_knobs.log)
TD void fast_push ( const Tracer& T, int*& top, uint32_t v ) {
    const uint32_t a = ( uint32_t ) ( uintptr_t ) top;
    // (bounds-checking builds: an entry beyond what the host planned -- LDS column + HBM part, the positive control's shrink taken off the column -- is refused and counted)
    if ( TERRA_CHECK_BOUNDS && ( int ) ( top - T.stack ) / TERRA_COL >= T.stack_cap + ( int ) T.spill_cap ) { if ( T.faults ) atomicAdd ( T.faults, 1ull ); return; }
    if ( __builtin_expect ( a < T.stack_lim, 1 ) ) *top = ( int ) v;
    else {
        const uint32_t k = ( a - T.stack_lim ) >> 10;
        if ( TERRA_CHECK_BOUNDS && ( !T.spill || k >= T.spill_cap ) ) { if ( T.faults ) atomicAdd ( T.faults, 1ull ); return; }
        T.spill[k] = v;
    }
    top += TERRA_COL;
}
TD uint32_t fast_pop ( const Tracer& T, int*& top ) {
    top -= TERRA_COL;
    const uint32_t a = ( uint32_t ) ( uintptr_t ) top;
    // (the LDS side is read through an LDS-typed pointer: left as two loads of generic pointers, the compiler merges them into ONE flat load of a selected address -- and a
    //  flat load goes through the texture addresser, the unit these kernels are short of, instead of the LDS pipeline)
    typedef const __attribute__ (( address_space ( 3 ) )) uint32_t* LdsPtr;
    if ( __builtin_expect ( a < T.stack_lim, 1 ) ) return * ( LdsPtr ) ( uintptr_t ) a;
    return T.spill[ ( a - T.stack_lim ) >> 10];
}
// compare-exchange of two (key, child word) pairs: afterwards a holds the smaller key
TD void order_pair ( uint32_t& ka, uint32_t& ca, uint32_t& kb, uint32_t& cb ) {
    const bool swap = kb < ka;
    const uint32_t k0 = swap ? kb : ka, k1 = swap ? ka : kb, c0 = swap ? cb : ca, c1 = swap ? ca : cb;
    ka = k0; kb = k1; ca = c0; cb = c1;
}
#define TERRA_FAST_ROOT_IN_HAND 0u
// (a leaf word in `hand` is recognised by ( int ) hand < -1: DEV_CHILD_EMPTY is -1 and no leaf word is -- a leaf has at most 4 triangles, so bits 29-30 of its count field are clear)
TD bool fast_traversing ( const Tracer& T, uint32_t hand, uint32_t held, const int* top ) { return ( hand != DEV_CHILD_EMPTY ) | ( top != T.stack ) | ( held != 0u ); }
template <int COUNT>
TD void traverse_fast_resume ( const Tracer& T, const Ray& ray, const RayState& st, V3 o_perm, ClosestRanked& best, int*& top, uint32_t& hand, uint32_t& held, int exit_active, Counters& c, bool checked = false, bool anyhit = false ) {
    const FastRay f = fast_ray ( ray, T.sc.fast_inv_scale );
    const char* nodes = reinterpret_cast<const char*> ( T.sc.fast_nodes_h );
    const float4* tris = reinterpret_cast<const float4*> ( T.sc.fast_tris );
    for ( ;; ) {
        // (the votes are taken on plain compares, whose results ARE wave masks; a vote on a combined bool costs a select + a compare to rebuild the mask)
        // a lane TESTS the leaf in `held` and may meanwhile descend on towards its next one (which then waits in hand): busy = can descend or holds
        const uint64_t m_hold = __builtin_amdgcn_ballot_w64 ( held != 0u ), m_can = __builtin_amdgcn_ballot_w64 ( ( int ) hand >= 0 ) | ( __builtin_amdgcn_ballot_w64 ( hand == DEV_CHILD_EMPTY ) & __builtin_amdgcn_ballot_w64 ( top != T.stack ) );
        const int n_can = __popcll ( m_can ), n_hold = __popcll ( m_hold ), n_busy = __popcll ( m_can | m_hold );
        if ( n_busy <= exit_active ) break;
        if ( n_can != 0 && n_hold * 16 < n_busy * TERRA_FAST_LEAF_16THS ) {
            if ( ( ( int ) hand >= 0 ) | ( ( hand == DEV_CHILD_EMPTY ) & ( top != T.stack ) ) ) {
                PS_WAVE ( c, kPsNodeIter ); PS_LANE ( c, kPsNodeLanes );
                uint32_t w = hand;
                if ( ( int ) w < 0 ) w = fast_pop ( T, top );
                uint32_t nw = w;                                     // (a leaf that waited on the stack stays in hand)
                if ( ( int ) w >= 0 ) {
                    const uint32_t off = w << 7;
                    const uint4 gx = *reinterpret_cast<const uint4*> ( nodes + ( off + f.px ) ), gy = *reinterpret_cast<const uint4*> ( nodes + ( off + f.py ) ),
                                gz = *reinterpret_cast<const uint4*> ( nodes + ( off + f.pz ) ), ch = *reinterpret_cast<const uint4*> ( nodes + ( off + 96u ) );      // {x0 x1 x2 x3} {y0 ..} {z0 ..} {children}
                    if ( COUNT ) ++c.nodes;
#if TERRA_PHASE_STATS
                    c.ps[kPsTop64] += w < 64u; c.ps[kPsTop256] += w < 256u; c.ps[kPsTop1024] += w < 1024u; c.ps[kPsTop4096] += w < 4096u;
#endif
                    const float limit_up = __uint_as_float ( __float_as_uint ( best.depth + 0.f ) + 1u );      // the next float up (FLT_MAX -> inf); + 0.f: a hit at depth -0 counts as +0
                    float te0, te1, te2, te3;
                    const bool hit0 = slab_half ( gx.x, gy.x, gz.x, f, limit_up, te0 );
                    const bool hit1 = slab_half ( gx.y, gy.y, gz.y, f, limit_up, te1 );
                    const bool hit2 = slab_half ( gx.z, gy.z, gz.z, f, limit_up, te2 );
                    const bool hit3 = slab_half ( gx.w, gy.w, gz.w, f, limit_up, te3 );
                    // nearest first: the entry distances (>= 0, so their bit patterns order like the floats) sorted with their child words; a box not entered sorts last
                    uint32_t k0 = hit0 ? __float_as_uint ( te0 ) : 0xffffffffu, k1 = hit1 ? __float_as_uint ( te1 ) : 0xffffffffu, k2 = hit2 ? __float_as_uint ( te2 ) : 0xffffffffu, k3 = hit3 ? __float_as_uint ( te3 ) : 0xffffffffu;
                    uint32_t c0 = ch.x, c1 = ch.y, c2 = ch.z, c3 = ch.w;
                    // (a full sorting network: finding only the nearest and pushing the others in slot order measured hall 218.9 -> 220.7 ms, sphere scene 318.6 -> 314.9;
                    //  profiles/r04_measurements/ab_fast_node_formats.log)
                    order_pair ( k0, c0, k1, c1 ); order_pair ( k2, c2, k3, c3 ); order_pair ( k0, c0, k2, c2 ); order_pair ( k1, c1, k3, c3 ); order_pair ( k1, c1, k2, c2 );
                    // the farthest goes in first, so the nearer ones come off first. (Branch-free pushes -- every child word stored at the top, the top moved only for the
                    // entered ones -- measured no faster on the hall and 2 % slower on the sphere scene: profiles/r04_measurements/ab_fast_tree_knobs.log)
                    if ( k3 != 0xffffffffu ) fast_push ( T, top, c3 );
                    if ( k2 != 0xffffffffu ) fast_push ( T, top, c2 );
                    if ( k1 != 0xffffffffu ) fast_push ( T, top, c1 );
#if TERRA_PHASE_STATS
                    if ( k1 != 0xffffffffu ) { const int dpt = ( int ) ( top - T.stack ) / TERRA_COL; ++c.ps[kPsCamLanes]; c.ps[kPsShadeIter] += dpt >= 4; c.ps[kPsRayLanes] += dpt >= 6; c.ps[kPsCamIter] += dpt >= 8; c.ps[kPsDrainIter] += dpt >= 12; c.ps[kPsShadeLanes] += dpt >= 16; }
#endif
                    nw = k0 != 0xffffffffu ? c0 : DEV_CHILD_EMPTY;
                }
                { const bool take = ( ( int ) nw < -1 ) & ( held == 0u ); held = take ? nw : held; nw = take ? DEV_CHILD_EMPTY : nw; }      // a leaf goes to the testing slot if that is free
                hand = nw;
            }
        } else if ( held != 0u ) {
            PS_WAVE ( c, kPsLeafIter ); PS_LANE ( c, kPsLeafLanes );
            const uint32_t ti = held & 0x07ffffffu;
            held = ( held & 0x78000000u ) ? held + 1u - 0x08000000u : 0u;        // next triangle of the leaf, one fewer to go
            if ( ( held == 0u ) & ( ( int ) hand < -1 ) ) { held = hand; hand = DEV_CHILD_EMPTY; }      // the leaf that waited in hand moves up
            const float4 a = tris[3 * ti], b = tris[3 * ti + 1], cc = tris[3 * ti + 2];          // three loads: every wave-level load instruction costs the texture addresser the same ~21 cycles
            const TriPerm tp = tri_perm ( a, b, cc, st );
            const uint32_t rank = __float_as_uint ( cc.w );
            if ( COUNT ) ++c.tri_tests;
            float depth;
            if ( watertight_permuted ( tp, o_perm, st, depth ) ) {
                if ( depth < best.depth || ( depth == best.depth && rank < best.rank ) ) {
                    if ( !checked || reference_reaches ( T, ti, ray ) ) {      // (checked: DevScene::reach, second pass)
                        best.depth = depth; best.rank = rank; best.tri = ti;
                        // a shadow ray that knows the triangle it expects (fast_expect), or an occlusion query (query_kernels.hip), only asks whether ANY triangle comes
                        // first: this one does, the lane is done. (With `checked` only a candidate the reference reaches ends the search; no render launch sets both.)
                        if ( anyhit ) { top = T.stack; hand = DEV_CHILD_EMPTY; held = 0u; }
                    }
                }
            }
        }
    }
}

// A ray of which only "is triangle E the closest hit" matters -- the light-sample ray of the Direct and MIS integrators (src/Terra.c:1349-1426: the sample counts when
// the ray's closest hit is the sampled light triangle) -- need not search for its closest hit. E is tested first, with the arithmetic the traversal would use on it; if
// the ray misses E the answer is no, whatever else it hits (false: the caller traces the ray the ordinary way, for the hit count). Otherwise the traversal starts from
// the closest hit (depth of E, rank of E): every box beyond E is culled from the first node on, and the first triangle that beats E -- nearer, or as near with a smaller
// reference visit rank: exactly the triangles the reference's traversal would have preferred -- ends it (traverse_fast_resume `anyhit`). best.tri stays
// TERRA_TRI_EXPECTED if none does. Scenes inside the coordinate range only (MODE 2: what the reference reaches needs no replay), kernels without work counters only
// (the attribute-fetch counter is defined by the CLOSEST hit's material). DevTri::pad of the soup holds the rank when the scene has a fast tree.
#define TERRA_TRI_EXPECTED 0xfffffffeu
TD bool fast_expect ( const Tracer& T, const RayState& st, V3 o_perm, uint32_t expected_soup, ClosestRanked& best ) {
    const float4* tris = reinterpret_cast<const float4*> ( T.sc.tris );
    const float4 a = tris[3 * expected_soup], b = tris[3 * expected_soup + 1], cc = tris[3 * expected_soup + 2];
    float depth;
    if ( !watertight_permuted ( tri_perm ( a, b, cc, st ), o_perm, st, depth ) ) return false;
    best.depth = depth; best.rank = __float_as_uint ( cc.w ); best.tri = TERRA_TRI_EXPECTED;
    return true;
}

// REACH = false: the kernels launched for scenes inside the coordinate range (template MODE 2) carry none of the replay code; MODE 3 = the same loops with it
template <int COUNT, bool REACH = true>
TD ClosestRanked bvh_traverse_fast ( const Tracer& T, const Ray& r, const RayState& st, Counters& c ) {
    V3 o_perm = permuted ( r.o, st );
    ClosestRanked best;
    // DevScene::reach: the closest of ALL hits is the answer if the reference would have reached it (then it is also the closest of the reachable ones);
    // only if not -- float rounding makes that very rare -- the ray is traced again with every candidate checked
    for ( int pass = 0; pass < 2; ++pass ) {
        best.depth = FLT_MAX; best.rank = 0xffffffffu; best.tri = 0xffffffffu;
        int* top = T.stack;
        uint32_t hand = TERRA_FAST_ROOT_IN_HAND, held = 0u;
        traverse_fast_resume<COUNT> ( T, r, st, o_perm, best, top, hand, held, 0, c, REACH && pass == 1 );
        if ( !REACH || pass == 1 || !T.sc.reach || best.tri == 0xffffffffu || reference_reaches ( T, best.tri, r ) ) break;
    }
    return best;
}
