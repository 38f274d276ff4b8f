// launch_plan.h -- how a launch is laid out: which traversal it takes, what it stages in LDS, how deep its stack and leaf list are, how many bytes of LDS, spill,
// job streams and job order it needs, how many blocks it launches. Plain host arithmetic, inline: the host layer (scene_host.cpp), the launchers in the .hip units
// and the CPU build of the host layer all run this one copy. The constants the device code reads too are in dev_types.h ("launch plan").
#pragma once
#include <hip/hip_runtime_api.h>
#include "dev_types.h"

// ---- shared pieces ----------------------------------------------------------------------------------------------------------
// compute units of the current device (256 where the runtime cannot say: no device, the CPU build)
inline uint32_t terra_cu_count ( void ) {
    int cus = 0, dev = 0; ( void ) hipGetDevice ( &dev );
    if ( hipDeviceGetAttribute ( &cus, hipDeviceAttributeMultiprocessorCount, dev ) != hipSuccess || cus < 1 ) { ( void ) hipGetLastError(); cus = 256; }
    return ( uint32_t ) cus;
}
// a deep stack: the leaf list shrinks, down to 4 entries, while the block (stack + list, 1 KB per entry, + other_bytes) asks for more than the 64 KB a launch may
// have without an opt-in; deeper still, the launch opts in (hipFuncAttributeMaxDynamicSharedMemorySize, one block per CU) up to terra_lds_block_limit
inline uint32_t terra_clamp_leaf_cap ( uint32_t stack_depth, uint32_t leaf_cap, size_t other_bytes ) {
    while ( leaf_cap > 4 && ( size_t ) ( stack_depth + leaf_cap ) * 1024 + other_bytes > ( size_t ) 64 * 1024 ) --leaf_cap;
    return leaf_cap;
}
// the reference tree with nothing staged and nothing parked (the AOV and query launchers): the whole stack in LDS, the leaf list takes what 64 KB leave
inline uint32_t terra_unstaged_leaf_cap ( uint32_t stack_depth, size_t other_bytes ) { return terra_clamp_leaf_cap ( stack_depth, TERRA_LEAF_CAP_MAX, other_bytes ); }
// bytes of stack spill (DevRenderParams::stack_spill) a grid of 256-thread blocks needs: spill_cap words per resident lane
inline size_t terra_spill_bytes ( size_t grid, uint32_t spill_cap ) { return grid * 256 * ( size_t ) spill_cap * sizeof ( uint32_t ); }
// the most a block may ask for (launch_instance opts in above 64 KB)
inline size_t terra_lds_block_limit ( void ) { return ( size_t ) TERRA_LDS_BLOCK_MAX_KB * 1024; }

// ---- blocks -----------------------------------------------------------------------------------------------------------------
inline uint32_t own_tiles ( uint32_t w, uint32_t h, uint32_t tile, uint32_t rank, uint32_t world ) {
    uint32_t tiles = ( ( w + tile - 1 ) / tile ) * ( ( h + tile - 1 ) / tile );
    return tiles > rank ? ( tiles - rank + world - 1 ) / world : 0;
}
// 256-thread blocks of one chunk (own tiles x blocks per tile)
inline uint32_t terra_render_blocks ( const DevRenderParams& p ) {
    uint32_t bpt = p.tile_size / 16;
    return own_tiles ( p.w, p.h, p.tile_size, p.rank, p.world ) * bpt * bpt;
}

// ---- LDS --------------------------------------------------------------------------------------------------------------------
// LDS a MODE-1 block spends on materials, lights and triangle areas (make_tracer): three sections, each a multiple of 16 bytes
inline size_t scene_extra_lds_bytes ( uint32_t n_objects, uint32_t n_lights, uint32_t n_tris ) {
    return ( ( ( size_t ) n_objects * sizeof ( DevMaterial ) + 15 ) & ~size_t ( 15 ) ) + ( size_t ) n_lights * sizeof ( DevLight ) + ( ( ( size_t ) n_tris * 4 + 15 ) & ~size_t ( 15 ) );
}
// the shading constants of a pair-form launch (dev_types.h "shading constants")
inline size_t terra_shade_consts_bytes ( const DevRenderParams& p ) {
    return ( p.lds_mode == 1 && p.leaf_rank && p.leaf_pairs ) ? ( size_t ) p.lds_tris * TERRA_SHADE_CONSTS_BYTES : 0;
}
// dynamic LDS per block of the planned launch
inline size_t terra_lds_bytes ( const DevRenderParams& p ) {
    return terra_shade_consts_bytes ( p ) + ( size_t ) ( p.stack_depth + p.leaf_cap + ( p.lds_mode == 1 ? TERRA_AUX_WORDS_LDS : TERRA_AUX_WORDS ) ) * 1024 + ( size_t ) p.lds_nodes * TERRA_LDS_NODE_BYTES + ( size_t ) p.lds_tris * ( 48 + 64 )
           + ( p.lds_mode == 1 ? scene_extra_lds_bytes ( p.scene.n_objects, p.scene.n_lights, p.scene.n_tris ) : 0 ) + ( p.lds_mode == 1 && p.leaf_rank ? ( p.leaf_pairs ? ( size_t ) terra_pair_section_bytes ( p.lds_tris / 2 ) : ( size_t ) p.lds_tris * 6 * 48 ) : 0 );      // (the leaf-box table of a flat launch rides in pad words of the ranked entries: no bytes of its own; the pair form's section includes its table)
}
// fast tree (MODE 2 / 3): nothing is staged. A lane holds at most two leaves (in registers: the one it tests, the next one), so there is no leaf list. The stack: its first TERRA_FAST_STACK_LDS entries
// in LDS (1 KB per entry and block), the rest -- up to the tree's worst case, which a ray almost never reaches -- in HBM, 4 bytes per entry and resident lane
// (DevRenderParams::stack_spill, part of the launch's scratch: traverse_fast.h fast_push / fast_pop). Depth no longer decides whether a tree can be launched.
// (Rounds 2-3 staged the first 64 nodes as plain 64-byte nodes read through a flat load: +3.7 % then. Flat loads go through the texture addresser like global ones,
// and that unit is what binds these kernels: nothing is gained by it now.)
// The plan of a fast-tree (MODE 2 / 3) launch: stack from the tree's depth, nothing staged
inline void terra_plan_fast_tree ( DevRenderParams& p ) {
    const uint32_t need = ( uint32_t ) ( p.scene.fast_max_stack < 1 ? 1 : p.scene.fast_max_stack );
    p.lds_mode = 2; p.lds_tris = 0; p.lds_nodes = 0; p.leaf_cap = 0; p.leaf_rank = 0; p.stack_depth = need < ( uint32_t ) TERRA_FAST_STACK_LDS ? need : ( uint32_t ) TERRA_FAST_STACK_LDS;
    p.spill_cap = need - p.stack_depth; p.stack_spill = nullptr;
}
// bytes of DevRenderParams::stack_spill a fast-tree launch needs (p.job_blocks set; 0: the stack fits in LDS): sized for the resident lanes such a launch can have
// at most (8 blocks of 256 threads per CU)
inline size_t terra_fast_spill_bytes ( const DevRenderParams& p ) {
    if ( p.lds_mode != 2 || p.spill_cap == 0 ) return 0;
    const size_t resident = ( size_t ) terra_cu_count() * 8;
    return terra_spill_bytes ( ( size_t ) p.job_blocks < resident ? ( size_t ) p.job_blocks : resident, p.spill_cap );
}

// LDS plan. Small scenes (whole scene + stack + a leaf list of at least TERRA_LEAF_CAP_RESIDENT_MIN entries <= budget): stage
// everything; with the Cornell box that is 31.9 KB per block (112-B staged nodes, 14-entry leaf list), so the 5 blocks/CU the
// Simple kernel's registers allow stay resident. The leaf list takes what the budget leaves, up to 16 entries: a list that
// fills is drained and the node loop resumes, so its length only decides how often that happens.
// Large scenes: nothing is staged -- their node fetches are bound by the L1 tag rate of divergent
// 16-byte loads (each lane its own 64-B node) and by latency, so resident blocks matter most: the
// leaf list takes what is left of the CU's 160 KB after fitting as many blocks as possible while
// keeping at least 8 entries (profiles/r01_measurements/ab4.log, ab5.log: 4 blocks x 14 entries 219 ms vs
// 3 blocks x 16 entries 305 ms vs 4-entry lists 261 ms on the 97k-triangle hall).
// leaf-list entries an LDS-resident plan can afford (0 = the scene does not fit)
inline uint32_t resident_leaf_cap ( uint32_t n_nodes, uint32_t n_tris, int max_stack, uint32_t n_objects, uint32_t n_lights ) {
    const uint32_t depth = max_stack < 1 ? 1u : ( uint32_t ) max_stack;
    const size_t fixed = ( size_t ) ( depth + TERRA_AUX_WORDS_LDS ) * 1024 + ( size_t ) n_nodes * TERRA_LDS_NODE_BYTES + ( size_t ) n_tris * 112 + scene_extra_lds_bytes ( n_objects, n_lights, n_tris );
    if ( fixed + ( size_t ) TERRA_LEAF_CAP_RESIDENT_MIN * 1024 > ( size_t ) TERRA_LDS_BUDGET ) return 0;
    const uint32_t cap = ( uint32_t ) ( ( ( size_t ) TERRA_LDS_BUDGET - fixed ) / 1024 );
    return cap > TERRA_LEAF_CAP_MAX ? TERRA_LEAF_CAP_MAX : cap;
}
// whole scene staged per block (the small-scene kernels)
inline bool terra_scene_fits_lds ( uint32_t n_nodes, uint32_t n_tris, int max_stack, uint32_t n_objects, uint32_t n_lights ) { return resident_leaf_cap ( n_nodes, n_tris, max_stack, n_objects, n_lights ) != 0; }
// fills stack_depth / lds_nodes / lds_tris / lds_mode / leaf_cap / leaf_rank
inline void terra_plan_lds ( DevRenderParams& p ) {
    uint32_t depth = p.scene.max_stack < 1 ? 1u : ( uint32_t ) p.scene.max_stack;
    p.stack_depth = depth;
    p.leaf_cap = TERRA_LEAF_CAP_MAX; p.leaf_rank = 0;
    if ( const uint32_t cap = resident_leaf_cap ( p.scene.n_nodes, p.scene.n_tris, p.scene.max_stack, p.scene.n_objects, p.scene.n_lights ) ) {
        p.lds_mode = 1; p.lds_nodes = p.scene.n_nodes; p.lds_tris = p.scene.n_tris; p.leaf_cap = cap;
        // at most TERRA_LEAF_RANK_MAX triangles: the leaf list gives way to the rank set and the permuted copies (traverse_ref.h "Ranked launches") if they
        // take no more LDS than the list did -- on the Cornell box 6 x 32 x 48 B = 9 KB in place of the list's 13 KB
        if ( p.scene.n_tris <= TERRA_LEAF_RANK_MAX && ( size_t ) p.scene.n_tris * 6 * 48 <= ( size_t ) cap * 1024 ) { p.leaf_rank = 1; p.leaf_cap = 0; }
        return;
    }
    p.lds_mode = 0; p.lds_nodes = 0; p.lds_tris = 0;
    for ( int blocks = 5; blocks >= 1; --blocks ) {
        int room = TERRA_LDS_CU_KB / blocks - ( int ) depth - TERRA_AUX_WORDS;       // KB per block left for the leaf list (2 KB of slack per CU)
        if ( room >= TERRA_LEAF_CAP_MIN || blocks == 1 ) { p.leaf_cap = ( uint32_t ) ( room > TERRA_LEAF_CAP_MAX ? TERRA_LEAF_CAP_MAX : ( room < 4 ? 4 : room ) ); break; }
    }
    // a deep tree: the block stays within 64 KB while the leaf list keeps at least 4 entries (terra_clamp_leaf_cap); beyond TERRA_LDS_BLOCK_MAX_KB the host
    // layer refuses the launch with a message (scene_host.cpp launch_render)
    p.leaf_cap = terra_clamp_leaf_cap ( p.stack_depth, p.leaf_cap, ( size_t ) TERRA_AUX_WORDS * 1024 );
}
// Flat leaf-box test: can a launch planned as p stage a table of n boxes? Ranked launches with the fused box test only (make_tracer stages under the same
// condition); the table rides in pad words of what such a launch stages anyway, one set per triangle, so it fits whenever n <= the triangles staged
inline bool terra_leaf_boxes_fit ( const DevRenderParams& p, uint32_t n ) {
    return n != 0 && n <= TERRA_LEAF_RANK_MAX && p.lds_mode == 1 && p.leaf_rank && p.leaf_cull && p.fused_slab && n <= p.lds_tris;
}

// ---- job streams and job order (render_kernels.hip "jobs", "job order") -------------------------------------------------------
// scratch of the job streams; 0: this launch keys its streams in the render kernel (p.lds_mode, p.job_blocks set)
inline size_t terra_job_streams_bytes ( const DevRenderParams& p ) { return p.lds_mode == 1 ? ( size_t ) p.job_blocks * 256 * 32 : 0; }
// launches of fewer pixel blocks keep the numbering's order (unless terra_amd_set_job_order(scene, 2))
inline uint32_t terra_job_order_min_blocks ( void ) { return TERRA_JOB_ORDER_MIN_BLOCKS; }
// scratch of the job order: class word + the two halves of the order per pixel block, or 0: this launch keeps the order of the numbering (p.job_blocks, p.lds_mode set);
// small_too: also below TERRA_JOB_ORDER_MIN_BLOCKS; ray_source: a ray-sourced launch (kernels.h terra_launch_render_rays) never has one -- the order and the empty
// skip that rides on it are made from camera rays
inline size_t terra_block_order_bytes ( const DevRenderParams& p, bool small_too, bool ray_source = false ) {
    if ( ray_source || terra_job_streams_bytes ( p ) == 0 || p.scene.n_tris == 0 || p.scene.n_tris > 4096 ) return 0;
    const size_t blocks = terra_render_blocks ( p );
    // (not for small launches -- below TERRA_JOB_ORDER_MIN_BLOCKS pixel blocks, a 256 x 256 rectangle: a tile-sized call is one of several in flight, whose work hides its tail,
    //  and its two extra small kernels would queue behind the other callers' render grids: the reference client's tile loop 66.5 -> 72.6 ms with them)
    return blocks >= ( small_too ? 1u : ( unsigned ) TERRA_JOB_ORDER_MIN_BLOCKS ) ? ( blocks * 3 * sizeof ( uint32_t ) + 255 ) & ~size_t ( 255 ) : 0;
}
